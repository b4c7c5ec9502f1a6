"""The fused soft code assignment (csrc/vq_soft.hip) away from the shapes of its golden fixtures: every one of the twelve
`vq_soft_assign_kernel<D, WANT_DIST, WANT_S>` instantiations, both row forms of phase B, K < 32, K = 1, N = 1, a full workgroup,
ragged last code tiles, buffers off 16-byte alignment, guard bands around every output, and the special values the kernel header
documents.  tests/test_soft_assign.py holds the fixtures; the restatement of both files is tests/_soft_ref.py.

Expected values: distances from the CPU oracle token by token (bit for bit), soft codes = `softmax64` of them, hard code = the
first-index argmin, drawn code = `draw(p, q)` outside `skip_set`.  Inputs: E = synth.codebook_trained(K, D, seed), x from
synth.z_tokens(seed + 1), q = torch.empty(N, K).exponential_(1) of a CPU generator seeded with seed + 2.

  case  D    K    N    temp  seed  what it reaches
  A     128  260  129  32    7501  16-byte rows, 9 code tiles with 4 codes in the last; a second phase-B stride of one lane; a second
                                   workgroup of one token
  B     128  67   33   8     7511  4-byte rows, a second phase-B stride of 3 lanes, a last tile of 3 codes, a second wave of one token
  C     64   7    31   4     7521  K < 32: one partial tile; one partial wave
  D     256  36   128  32    7531  exactly one full workgroup
  E     128  1    5    1     7541  K = 1: soft exactly 1.0f, code 0, draw 0
  F     64   160  1    16    7551  N = 1
  G     256  260  129  32    7561  A at D = 256
  H     64   67   33   8     7571  B at D = 64
  P     96   100  70   8     7581  a padded width: D = 96 runs at 128, bit for bit what explicit zero padding gives

Each case runs through every way the entry point can be asked (FORMS); `test_case_table_reaches_what_it_claims` restates the
launcher's choice of (D, WANT_DIST, WANT_S, V) for every call the GPU tests make and finds all twelve instantiations, and both row
forms at every width and WANT_DIST where phase B runs, without a device.

Tolerance of the soft codes, per case: max(4 e_ref, 4 ulp32(largest p)), e_ref = the distance of torch's own fp32 CPU softmax of
the same scores from `softmax64` (_soft_ref.soft_allowance).  Row sums: within K times that of 1.  Everything else is an equality:
distances against the oracle, hard codes across forms and against vq_assign, soft across forms and runs, the draw with and without
the soft output.  The two row forms sum a row in different lane orders, so across them soft is compared within the allowance.

What the cases see.  Two mistakes that stay in bounds were tried on a scratch build.  Phase B's sum taken over a lane's first
piece of the row only: the soft bound fails in A, B, G, H (forms and guard bands), in A, F, G, P off alignment (their K exceeds 64,
one stride of the 4-byte rows), in the list quantizer and the RQ test; C, D, E and the aligned F and P have a single stride and pass.
The merge of a token's 32 lanes taking the last index among equal distances and ignoring NaN: only test_special_values fails
(the duplicated codebook rows and the first NaN of the token with an infinite channel); the table's cases hold no tie."""
import collections
import os
import re

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib, synth
from tests import _soft_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

Case = collections.namedtuple("Case", "D K N temp seed claims")
CASES = {
    "A": Case(128, 260, 129, 32.0, 7501, {"v4", "ragged_tile", "second_stride", "second_workgroup", "partial_wave"}),
    "B": Case(128, 67, 33, 8.0, 7511, {"v1", "ragged_tile", "second_stride", "partial_wave"}),
    "C": Case(64, 7, 31, 4.0, 7521, {"v1", "k<32", "ragged_tile", "partial_wave"}),
    "D": Case(256, 36, 128, 32.0, 7531, {"v4", "ragged_tile", "full_workgroup"}),
    "E": Case(128, 1, 5, 1.0, 7541, {"v1", "k=1", "k<32", "partial_wave"}),
    "F": Case(64, 160, 1, 16.0, 7551, {"v4", "n=1", "partial_wave"}),
    "G": Case(256, 260, 129, 32.0, 7561, {"v4", "ragged_tile", "second_stride", "second_workgroup", "partial_wave"}),
    "H": Case(64, 67, 33, 8.0, 7571, {"v1", "ragged_tile", "second_stride", "partial_wave"}),
    "P": Case(96, 100, 70, 8.0, 7581, {"v4", "padded", "ragged_tile", "partial_wave"}),
}
NAMES = tuple(CASES)
ALIGNED_K = tuple(n for n in NAMES if CASES[n].K % 4 == 0)        # the cases an offset of 4 bytes moves to the 4-byte rows

# what a call asks for: (soft, dist, q).  `dist` alone is not reachable through quantize.soft_assign: the C entry point directly.
Form = collections.namedtuple("Form", "soft dist q")
FORMS = {
    "soft+dist": Form(True, True, False),        # <true, true>
    "soft": Form(True, False, False),            # <false, true>
    "dist": Form(False, True, False),            # <true, false>
    "codes": Form(False, False, False),          # <false, false>
    "soft+q": Form(True, False, True),           # phase B with the draw
    "q": Form(False, False, True),               # the scores in the workspace
}
GUARD_FORMS = (Form(True, True, False), Form(True, True, True), Form(False, True, True), Form(False, False, True))
SENTINEL = 0x5A5AA5A5

_CACHE = {}


def _cached(key, make):
    """computed once, shared by the tests that need it and never written to afterwards"""
    if key not in _CACHE:
        val = make()
        for a in (val.values() if isinstance(val, dict) else [val]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def _padded(a, Dp):
    out = np.zeros((a.shape[0], Dp), np.float32)
    out[:, :a.shape[1]] = a
    return out


def _expected(oracle_mod, x, E, q, temp):
    """the oracle's distances token by token and the restatement of everything derived from them"""
    dist = np.stack([oracle_mod.token_distances(x[n], E) for n in range(x.shape[0])])
    p = R.softmax64(dist, temp)
    out = {"dist": dist, "p": p, "hard": np.argmin(dist, axis=1).astype(np.int64)}
    if q is not None:
        out["drawn"], out["skip"] = R.draw(p, q), R.skip_set(p, q)
    return out


def _inputs(name, oracle_mod):
    c = CASES[name]

    def make():
        E = synth.codebook_trained(c.K, c.D, seed=c.seed)
        x = np.ascontiguousarray(synth.z_tokens(E, 1, c.N, 1, c.seed + 1)[0, :, :, 0].T)
        q = torch.empty(c.N, c.K).exponential_(1, generator=torch.Generator().manual_seed(c.seed + 2)).numpy()
        Dp = R.kernel_form(c.D, c.K, True, False, False)[0]
        out = {"E": E, "x": x, "q": q}
        out.update(_expected(oracle_mod, _padded(x, Dp), _padded(E, Dp), q, c.temp))
        out["e_ref"] = R.softmax32_error(out["dist"], c.temp)
        out["allow"] = R.soft_allowance(out["dist"], c.temp)
        return out

    return _cached(("inputs", name), make)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- CPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_restatement_and_skip_share(name, oracle_mod):
    """the restatement alone: rows sum to 1, the skip share is within the cap of tests/test_soft_assign.py (1 % of the tokens),
    the allowance is the rule of the module docstring and not a number taken from the kernel"""
    c, inp = CASES[name], _inputs(name, oracle_mod)
    assert inp["dist"].shape == (c.N, c.K) and np.isfinite(inp["dist"]).all()
    assert np.abs(inp["p"].sum(1) - 1.0).max() <= 1e-12
    assert inp["skip"].mean() <= 0.01
    assert inp["allow"] == max(4.0 * inp["e_ref"], 4.0 * R.ulp32(inp["p"].max()))
    assert 0.0 < inp["allow"] <= 4e-6                               # an fp32 softmax is never further off than this
    print("%s: e_ref %.3g, largest p %.3g, allowance %.3g, skip share %.3g" % (name, inp["e_ref"], inp["p"].max(), inp["allow"], inp["skip"].mean()))
    if c.K == 1:
        assert inp["e_ref"] == 0.0 and (inp["p"] == 1.0).all() and not inp["drawn"].any() and not inp["skip"].any()
    if c.D == 96:                                                   # zero channels change no bit of a distance
        d96 = np.stack([oracle_mod.token_distances(inp["x"][n], inp["E"]) for n in range(c.N)])
        assert np.array_equal(_bits(d96), _bits(inp["dist"]))


def test_restatement_self_checks():
    d = np.array([[1.0, 2.0, 4.0], [np.nan, 0.0, 1.0], [np.inf, np.inf, np.inf], [0.5, np.inf, 0.5]], np.float32)
    p = R.softmax64(d, 2.0)
    e = np.exp(-np.array([0.0, 0.5, 1.5]))
    assert np.abs(p[0] - e / e.sum()).max() <= 1e-15
    assert np.isnan(p[1]).all() and np.isnan(p[2]).all()            # a NaN distance, and a row maximum of -inf
    assert np.array_equal(p[3], [0.5, 0.0, 0.5])
    q = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [1.0, 1.0, 0.0]], np.float32)
    assert np.array_equal(R.draw(p, q), [0, 0, 0, 2])               # NaN rows draw 0; p / 0 = inf wins
    assert np.isnan(R.softmax64(40 * d[:1], 1e-37)).all()           # every score overflows to -inf
    assert np.array_equal(R.softmax64(d[:1], 1e-6), [[1.0, 0.0, 0.0]])
    assert not R.skip_set(np.ones((3, 1)), np.ones((3, 1))).any()   # one code: nothing to flip to
    assert R.skip_set(np.array([[0.5, 0.5]]), np.array([[1.0, 1.0 + 1e-6]])).all()
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(0.3) == 2.0 ** -25
    assert R.kernel_form(96, 100, True, False, False) == (128, False, True, 4)
    assert R.kernel_form(64, 100, True, True, True, aligned=False) == (64, True, True, 1)
    assert R.kernel_form(256, 7, False, True, False) == (256, True, False, None)


def _calls():
    """(D, K, soft, dist, q, aligned) of every kernel launch the GPU tests of this file make through the entry point"""
    out = []
    for name in NAMES:
        c = CASES[name]
        out += [(c.D, c.K, f.soft, f.dist, f.q, True) for f in FORMS.values()]                  # test_forms
        out += [(c.D, c.K, f.soft, f.dist, f.q, True) for f in GUARD_FORMS]                     # test_guard_bands
    for name in ALIGNED_K:
        c = CASES[name]
        out += [(c.D, c.K, f.soft, f.dist, f.q, False) for f in GUARD_FORMS]                    # test_off_alignment
    return out


def test_case_table_reaches_what_it_claims():
    src = open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "vq_soft.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    hint = " -- vq_soft.hip changed its launch rule: rebuild the case table of tests/test_soft_assign_shapes.py for it"
    for line in ("const uintptr_t bits = (uintptr_t)sbuf | (uintptr_t)soft | (uintptr_t)q;",
                 "const int vec = (K % 4 == 0) && (bits & 15) == 0;",
                 "const dim3 grid((unsigned)((N + 127) / 128)), block(256);",
                 "if (dist != nullptr && sbuf != nullptr) return dvq_launch_lds<vq_soft_assign_kernel<D, true, true>>",
                 "if (dist != nullptr) return dvq_launch_lds<vq_soft_assign_kernel<D, true, false>>",
                 "if (sbuf != nullptr) return dvq_launch_lds<vq_soft_assign_kernel<D, false, true>>",
                 "for (int j = lane * V; j < K; j += 64 * V)",
                 "case 64: return launch_soft<64>", "case 128: return launch_soft<128>", "case 256: return launch_soft<256>"):
        assert line in flat, line + hint
    abi = re.sub(r"\s+", " ", open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "dvq_abi.hip")).read())
    assert "float *sbuf = soft; if (!soft && q) {" in abi and "sbuf = (float *)ws;" in abi, hint
    forms = {R.kernel_form(*call) for call in _calls()}
    kernels = {f[:3] for f in forms}
    assert kernels == {(D, wd, ws) for D in (64, 128, 256) for wd in (False, True) for ws in (False, True)} and len(kernels) == 12
    for D in (64, 128, 256):
        for wd in (False, True):
            assert {f[3] for f in forms if f[:3] == (D, wd, True)} == {1, 4}, (D, wd)
            assert {f[3] for f in forms if f[:3] == (D, wd, False)} == {None}, (D, wd)
    reached = set()
    for name, c in CASES.items():
        Dp, _, _, V = R.kernel_form(c.D, c.K, True, False, False)
        claims = {"v%d" % V}
        if Dp != c.D:
            claims.add("padded")
        if c.K % 32:
            claims.add("ragged_tile")                             # the last code tile holds K % 32 codes
        if c.K < 32:
            claims.add("k<32")
        if c.K == 1:
            claims.add("k=1")
        if c.K > 64 * V:
            claims.add("second_stride")                           # a lane of phase B takes a second piece of the row
        if c.N % 128 == 0:
            claims.add("full_workgroup")
        if c.N > 128:
            claims.add("second_workgroup")
        if c.N % 32:
            claims.add("partial_wave")
        if c.N == 1:
            claims.add("n=1")
        assert c.claims <= claims, (name, c.claims - claims)
        reached |= c.claims
    assert reached == {"v1", "v4", "padded", "ragged_tile", "k<32", "k=1", "second_stride", "full_workgroup", "second_workgroup",
                       "partial_wave", "n=1"}
    a, b = CASES["A"], CASES["B"]
    assert (a.K + 31) // 32 == 9 and a.K - 256 == 4 and a.N - 128 == 1                # one lane of four codes in the second stride
    assert b.K - 64 == 3 and b.K % 32 == 3 and b.N - 32 == 1
    assert any(c.K % 4 == 0 and c.K % 32 != 0 for c in CASES.values())                # 16-byte rows end inside a ragged tile
    assert any(c.K % 4 != 0 and c.K > 64 for c in CASES.values())                     # 4-byte rows take a second stride


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _t(dev):
    return lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)            # a copy: the cached inputs are read-only


def _off_alignment(a):
    """a contiguous copy of the tensor that starts one float behind a 16-byte boundary"""
    buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=a.device)
    v = buf[1:].view(a.shape)
    v.copy_(a)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def _run(dev, x, E, temp, form, q=None, prep=None):
    """(soft, codes, dist) as numpy (None where not asked for) of one call; x, E, q: tensors on the device or numpy arrays"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, soft_assign
    t = lambda a: a if isinstance(a, torch.Tensor) else _t(dev)(a)
    x, E = t(x), t(E)
    q = t(q) if form.q else None
    prep = _CodebookPrep() if prep is None else prep
    if form.soft or form.q or not form.dist:
        soft, codes, dist = soft_assign(x, E, prep, temp, q, form.soft, form.dist)
    else:                                                           # distances alone: soft = NULL, q = NULL
        N, D, K = x.shape[0], x.shape[1], E.shape[0]
        if D not in (64, 128, 256):
            Dp = R.kernel_form(D, K, False, True, False)[0]
            xp, Ep = x.new_zeros((N, Dp)), E.new_zeros((K, Dp))
            xp[:, :D], Ep[:, :D] = x, E
            x, E, D = xp, Ep, Dp
        soft, dist = None, torch.full((N, K), float("nan"), device=dev)
        codes = torch.full((N,), -7, dtype=torch.int64, device=dev)
        _lib.checked.dvq_vq_soft_assign_flat_f32(x.data_ptr(), E.data_ptr(), prep.get(E).data_ptr(), N, D, K, float(temp), 0, 0,
                                                 dist.data_ptr(), codes.data_ptr(), 0, 0, _lib.stream_ptr(dev))
    n = lambda a: None if a is None else a.cpu().numpy()
    return n(soft), n(codes), n(dist)


def _check_soft(what, soft, inp, K):
    err = float(np.abs(soft.astype(np.float64) - inp["p"]).max())
    rows = float(np.abs(soft.astype(np.float64).sum(1) - 1.0).max())
    print("%s: soft error %.3g (allowance %.3g, e_ref %.3g), row sums within %.3g" % (what, err, inp["allow"], inp["e_ref"], rows))
    assert err <= inp["allow"], what
    assert rows <= K * inp["allow"], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_forms(name, dev, oracle_mod):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, _CodebookPrep, vq_assign
    c, inp = CASES[name], _inputs(name, oracle_mod)
    t = _t(dev)
    x, E, q = t(inp["x"]), t(inp["E"]), t(inp["q"])
    res = {f: _run(dev, x, E, c.temp, form, q) for f, form in FORMS.items()}
    again = {f: _run(dev, x, E, c.temp, form, q) for f, form in FORMS.items()}
    for f, form in FORMS.items():
        soft, codes, dist = res[f]
        assert (soft is not None) == form.soft and (dist is not None) == form.dist, f
        assert codes.shape == (c.N,) and codes.dtype == np.int64, f
        if form.dist:
            assert dist.shape == (c.N, c.K) and np.array_equal(_bits(dist), _bits(inp["dist"])), f
        if form.soft:
            assert soft.shape == (c.N, c.K) and np.array_equal(_bits(soft), _bits(res["soft+dist"][0])), f
            assert np.array_equal(_bits(soft), _bits(again[f][0])), f
        if not form.q:
            assert np.array_equal(codes, inp["hard"]), f
        assert np.array_equal(codes, again[f][1]), f
    _check_soft("%s (D=%d K=%d N=%d temp=%g)" % (name, c.D, c.K, c.N, c.temp), res["soft+dist"][0], inp, c.K)
    assert np.array_equal(vq_assign(x, E, _CodebookPrep(), want_zq=False, want_loss=False)[1].cpu().numpy(), inp["hard"])
    keep = ~inp["skip"]
    assert np.array_equal(res["soft+q"][1], res["q"][1])
    assert np.array_equal(res["q"][1][keep], inp["drawn"][keep])
    if c.K == 1:
        assert (res["soft"][0] == np.float32(1.0)).all() and not res["q"][1].any() and not res["codes"][1].any()
    # the module: the same bits; its draw takes q from torch's generator as this test draws it
    m = VectorQuantize2(c.K, c.D, accept_image_fmap=False, channel_last=True).to(dev).eval()
    m.codebook.weight.data[:-1].copy_(E)
    m.invalidate_codebook_cache()
    soft_m, code_m = m.get_soft_codes(x, temp=c.temp)
    assert np.array_equal(_bits(soft_m.cpu().numpy()), _bits(res["soft"][0])) and np.array_equal(code_m.cpu().numpy(), inp["hard"])
    torch.manual_seed(c.seed)
    q_m = torch.empty(c.N, c.K, dtype=torch.float32, device=dev).exponential_(1)
    torch.manual_seed(c.seed)
    soft_s, code_s = m.get_soft_codes(x, temp=c.temp, stochastic=True)
    want = _run(dev, x, E, c.temp, FORMS["soft+q"], q_m)
    assert np.array_equal(_bits(soft_s.cpu().numpy()), _bits(want[0])) and np.array_equal(code_s.cpu().numpy(), want[1])
    skip_m = R.skip_set(inp["p"], q_m.cpu().numpy())
    assert np.array_equal(want[1][~skip_m], R.draw(inp["p"], q_m.cpu().numpy())[~skip_m])


@pytest.mark.gpu
def test_padded_width_equals_explicit_padding(dev, oracle_mod):
    c, inp = CASES["P"], _inputs("P", oracle_mod)
    xp, Ep = _padded(inp["x"], 128), _padded(inp["E"], 128)
    for f, form in FORMS.items():
        a = _run(dev, inp["x"], inp["E"], c.temp, form, inp["q"])
        b = _run(dev, xp, Ep, c.temp, form, inp["q"])
        for u, v in zip(a, b):
            assert (u is None) == (v is None), f
            assert u is None or np.array_equal(u.view(np.uint32 if u.dtype == np.float32 else np.int64),
                                               v.view(np.uint32 if v.dtype == np.float32 else np.int64)), f


def _views(dev, x, q):
    """the same values behind non-contiguous (transposed) views"""
    t = _t(dev)
    xv, qv = t(x.T).t(), t(q.T).t()
    assert x.shape[0] == 1 or not (xv.is_contiguous() or qv.is_contiguous())
    return xv, qv


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALIGNED_K)
def test_off_alignment(name, dev, oracle_mod):
    """K % 4 == 0 with q, soft or the row start 4 bytes off a 16-byte boundary: the 4-byte rows.  Against the aligned call: soft
    within the allowance (the row forms sum in different lane orders), codes equal outside the skip set, distances the same bits"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    c, inp = CASES[name], _inputs(name, oracle_mod)
    t = _t(dev)
    x, E, q = t(inp["x"]), t(inp["E"]), t(inp["q"])
    keep = ~inp["skip"]
    base = _run(dev, x, E, c.temp, Form(True, True, True), q)
    q_off = _off_alignment(q)
    # through the wrapper: q alone is off
    for form in (Form(True, True, True), Form(False, False, True)):
        soft, codes, dist = _run(dev, x, E, c.temp, form, q_off)
        assert np.array_equal(codes[keep], inp["drawn"][keep]) and np.array_equal(codes[keep], base[1][keep])
        if form.soft:
            _check_soft("%s with q off alignment" % name, soft, inp, c.K)
            assert np.abs(soft.astype(np.float64) - base[0]).max() <= inp["allow"]
            assert np.array_equal(_bits(dist), _bits(inp["dist"]))
    # through the C entry point: soft (and dist) 4 bytes off, q aligned and absent; the workspace form with q off
    prep = _CodebookPrep()
    Dp = R.kernel_form(c.D, c.K, True, False, False)[0]
    xk, Ek = t(_padded(inp["x"], Dp)), t(_padded(inp["E"], Dp))
    pbuf = prep.get(Ek)
    nws = _lib.checked.dvq_vq_soft_assign_workspace_bytes(c.N, Dp, c.K)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)
    for form in GUARD_FORMS:
        soft = _off_alignment(torch.zeros(c.N, c.K, device=dev)) if form.soft else None
        dist = _off_alignment(torch.zeros(c.N, c.K, device=dev)) if form.dist else None
        qq = None if not form.q else (q if form.soft else q_off)    # without soft the workspace is aligned: q carries the offset
        codes = torch.full((c.N,), -7, dtype=torch.int64, device=dev)
        assert R.kernel_form(c.D, c.K, form.soft, form.dist, form.q, aligned=False)[3] == 1
        use_ws = form.q and not form.soft
        _lib.checked.dvq_vq_soft_assign_flat_f32(xk.data_ptr(), Ek.data_ptr(), pbuf.data_ptr(), c.N, Dp, c.K, c.temp, _lib.ptr(qq),
                                                 _lib.ptr(soft), _lib.ptr(dist), codes.data_ptr(), ws.data_ptr() if use_ws else 0,
                                                 nws if use_ws else 0, _lib.stream_ptr(dev))
        codes = codes.cpu().numpy()
        if form.q:
            assert np.array_equal(codes[keep], inp["drawn"][keep]), form
        else:
            assert np.array_equal(codes, inp["hard"]), form
        if form.dist:
            assert np.array_equal(_bits(dist.cpu().numpy()), _bits(inp["dist"])), form
        if form.soft:
            _check_soft("%s with soft off alignment, %s" % (name, "q" if form.q else "no q"), soft.cpu().numpy(), inp, c.K)
            assert np.abs(soft.cpu().numpy().astype(np.float64) - base[0]).max() <= inp["allow"]
    # non-contiguous x and q: the wrapper's copies are aligned, so the same bits as the plain call
    xv, qv = _views(dev, inp["x"], inp["q"])
    got = _run(dev, xv, E, c.temp, Form(True, True, True), qv)
    assert all(np.array_equal(u, v) for u, v in zip(got, base))


@pytest.mark.gpu
def test_leading_dimensions(dev, oracle_mod):
    """x [2, 3, 21, D] and q [2, 3, 21, K]: outputs in the leading shape, rows the bits of the flat call"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, soft_assign
    c, inp = CASES["A"], _inputs("A", oracle_mod)
    t = _t(dev)
    n = 126
    x, E, q = t(inp["x"][:n]), t(inp["E"]), t(inp["q"][:n])
    soft, codes, dist = soft_assign(x.view(2, 3, 21, c.D), E, _CodebookPrep(), c.temp, q.view(2, 3, 21, c.K), True, True)
    assert soft.shape == (2, 3, 21, c.K) and dist.shape == (2, 3, 21, c.K) and codes.shape == (2, 3, 21)
    flat = _run(dev, inp["x"], E, c.temp, Form(True, True, True), inp["q"])
    assert np.array_equal(_bits(soft.cpu().numpy().reshape(n, c.K)), _bits(flat[0][:n]))
    assert np.array_equal(codes.cpu().numpy().reshape(n), flat[1][:n])
    assert np.array_equal(_bits(dist.cpu().numpy().reshape(n, c.K)), _bits(inp["dist"][:n]))


def _guarded(numel, pad, dtype, dev):
    """a buffer of pad + numel + pad words filled with the sentinel pattern, and the window in its middle"""
    word = SENTINEL if dtype == torch.int32 else (SENTINEL << 32) | SENTINEL
    buf = torch.full((2 * pad + numel,), word, dtype=dtype, device=dev)
    return buf, buf[pad:pad + numel]


def _intact(buf, lo, hi):
    """every word of the buffer outside [lo, hi) still holds the sentinel pattern (compared as integers)"""
    a = buf.cpu().numpy()
    word = SENTINEL if a.dtype == np.int32 else (SENTINEL << 32) | SENTINEL
    return bool((a[:lo] == word).all() and (a[hi:] == word).all())


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_guard_bands(name, dev, oracle_mod):
    """soft, dist, codes and the workspace in the middle of larger buffers filled with a sentinel pattern, at least N x K words
    before and after: every word outside the [N, K] and [N] windows keeps its bits"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    c, inp = CASES[name], _inputs(name, oracle_mod)
    t = _t(dev)
    Dp = R.kernel_form(c.D, c.K, True, False, False)[0]
    x, E, q = t(_padded(inp["x"], Dp)), t(_padded(inp["E"], Dp)), t(inp["q"])
    pbuf = _CodebookPrep().get(E)
    NK = c.N * c.K
    pad = (NK + 63) // 64 * 64                                      # the windows stay 256-byte aligned
    cpad = (c.N + 31) // 32 * 32
    nws = _lib.checked.dvq_vq_soft_assign_workspace_bytes(c.N, Dp, c.K)
    assert nws >= NK * 4
    keep = ~inp["skip"]
    for form in GUARD_FORMS:
        soft_b, soft = _guarded(NK, pad, torch.int32, dev)
        dist_b, dist = _guarded(NK, pad, torch.int32, dev)
        ws_b, ws = _guarded(nws // 4, pad, torch.int32, dev)
        codes_b, codes = _guarded(c.N, cpad, torch.int64, dev)
        assert soft.data_ptr() % 256 == 0 and ws.data_ptr() % 256 == 0
        use_ws = form.q and not form.soft
        _lib.checked.dvq_vq_soft_assign_flat_f32(
            x.data_ptr(), E.data_ptr(), pbuf.data_ptr(), c.N, Dp, c.K, c.temp, q.data_ptr() if form.q else 0,
            soft.data_ptr() if form.soft else 0, dist.data_ptr() if form.dist else 0, codes.data_ptr(),
            ws.data_ptr() if use_ws else 0, nws if use_ws else 0, _lib.stream_ptr(dev))
        torch.cuda.synchronize()
        # outside the windows; a buffer that was not passed keeps every word
        assert _intact(soft_b, pad, pad + (NK if form.soft else 0)), form
        assert _intact(dist_b, pad, pad + (NK if form.dist else 0)), form
        assert _intact(codes_b, cpad, cpad + c.N), form
        # the workspace: nothing before it, nothing behind its first N K words (the rest of its 256-byte rounding included)
        assert _intact(ws_b, pad, pad + (NK if use_ws else 0)), form
        # inside: what the plain call gives
        got_codes = codes.cpu().numpy()
        if form.q:
            assert np.array_equal(got_codes[keep], inp["drawn"][keep]), form
        else:
            assert np.array_equal(got_codes, inp["hard"]), form
        if form.dist:
            assert np.array_equal(dist.cpu().numpy().view(np.uint32).reshape(c.N, c.K), _bits(inp["dist"])), form
        if form.soft:
            _check_soft("%s in guard bands" % name, soft.cpu().numpy().view(np.float32).reshape(c.N, c.K), inp, c.K)


@pytest.mark.gpu
@pytest.mark.parametrize("order", ("large_first", "small_first"))
def test_workspace_of_another_shape(order, dev, oracle_mod):
    """the draw without the soft output parks its scores in a workspace the prepared codebook caches: a large case and then a
    small one through the same object, and the other way round"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    c, inp = CASES["A"], _inputs("A", oracle_mod)
    t = _t(dev)
    E = t(inp["E"])
    prep = _CodebookPrep()
    small = 5
    sizes = (c.N, small) if order == "large_first" else (small, c.N)
    keep = ~inp["skip"]
    for n in sizes + sizes:
        _, codes, _ = _run(dev, inp["x"][:n], E, c.temp, FORMS["q"], inp["q"][:n], prep=prep)
        assert np.array_equal(codes[keep[:n]], inp["drawn"][:n][keep[:n]]), (order, n)
        _, fresh, _ = _run(dev, inp["x"][:n], E, c.temp, FORMS["q"], inp["q"][:n])
        assert np.array_equal(codes, fresh), (order, n)
    assert len([k for k in prep._ws if k[4] == "soft"]) == 2


# ---- special values ---------------------------------------------------------------------------------------------------------

SP_D, SP_K, SP_N, SP_TEMP = 64, 40, 40, 8.0
SP_NAN, SP_INF, SP_EQUAL, SP_ZERO, SP_QZERO, SP_ORDINARY = 3, 9, 17, 33, 21, 5      # token rows
SP_DUP, SP_HUGE = (6, 30), 12                                                       # codebook rows


def _special(oracle_mod):
    def make():
        E = synth.codebook_trained(SP_K, SP_D, seed=7601)
        E[SP_DUP[1]] = E[SP_DUP[0]]
        E[SP_HUGE] = np.float32(1e20)                               # |e|^2 = +inf, every dot finite
        x = np.ascontiguousarray(synth.z_tokens(E[:SP_HUGE], 1, SP_N, 1, 7602)[0, :, :, 0].T)
        x[SP_NAN, 5] = np.nan
        x[SP_INF, 11] = np.inf
        x[SP_EQUAL] = E[SP_DUP[0]]                                  # equal to a codebook row that has a duplicate: the first wins
        x[SP_ZERO] = 0.0
        q = torch.empty(SP_N, SP_K).exponential_(1, generator=torch.Generator().manual_seed(7603)).numpy()
        out = {"E": E, "x": x}
        exp = _expected(oracle_mod, x, E, q, SP_TEMP)
        j = int(np.argsort(exp["p"][SP_QZERO])[-3])                 # a code with p > 0 that is not the likeliest
        q[SP_QZERO, j] = 0.0
        out.update(_expected(oracle_mod, x, E, q, SP_TEMP))
        out["q"], out["qzero_code"] = q, j
        return out

    return _cached(("special",), make)


def test_special_values_restated(oracle_mod):
    """what the special rows are expected to give, from the oracle's distances and the restatement alone"""
    sp = _special(oracle_mod)
    d, p = sp["dist"], sp["p"]
    assert np.isnan(d[SP_NAN]).all() and np.isnan(p[SP_NAN]).all() and sp["hard"][SP_NAN] == 0 and sp["drawn"][SP_NAN] == 0
    # an infinite channel: the dot is +-inf, the distance +inf or inf - inf = NaN; the NaN is the argmin and the row is NaN
    assert np.isnan(d[SP_INF]).any() and (np.isnan(d[SP_INF]) | (d[SP_INF] == np.inf)).all() and np.isnan(p[SP_INF]).all()
    assert sp["hard"][SP_INF] == int(np.flatnonzero(np.isnan(d[SP_INF]))[0]) and sp["drawn"][SP_INF] == 0
    rest = np.setdiff1d(np.arange(SP_N), [SP_NAN, SP_INF])
    assert (d[rest, SP_HUGE] == np.inf).all() and (p[rest, SP_HUGE] == 0.0).all()
    assert np.isfinite(np.delete(d[rest], SP_HUGE, axis=1)).all() and np.isfinite(p[rest]).all()
    assert sp["hard"][SP_EQUAL] == SP_DUP[0] and d[SP_EQUAL, SP_DUP[0]] == d[SP_EQUAL, SP_DUP[1]]
    assert np.array_equal(_bits(d[:, SP_DUP[0]][rest]), _bits(d[:, SP_DUP[1]][rest]))
    assert sp["q"][SP_QZERO, sp["qzero_code"]] == 0.0 and p[SP_QZERO, sp["qzero_code"]] > 0
    assert sp["drawn"][SP_QZERO] == sp["qzero_code"] != sp["hard"][SP_QZERO]
    assert sp["skip"].mean() <= 0.01 and not sp["skip"][[SP_NAN, SP_INF, SP_QZERO]].any()


def _same_where_not_nan(got, ref):
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan)) and np.array_equal(_bits(np.where(nan, np.float32(0), got)),
                                                                       _bits(np.where(nan, np.float32(0), ref)))


@pytest.mark.gpu
def test_special_values(dev, oracle_mod):
    """a NaN distance is the argmin and makes the row NaN; all ratios NaN draw 0; an infinite code norm gives p = 0 exactly;
    duplicated rows: the first index; q = 0 at a code with p > 0 draws that code"""
    sp = _special(oracle_mod)
    finite = np.setdiff1d(np.arange(SP_N), [SP_NAN, SP_INF])
    allow = max(R.soft_allowance(sp["dist"][finite], SP_TEMP), 0.0)
    keep = ~sp["skip"]
    for f, form in FORMS.items():
        soft, codes, dist = _run(dev, sp["x"], sp["E"], SP_TEMP, form, sp["q"])
        if form.dist:
            assert _same_where_not_nan(dist, sp["dist"]), f
        if form.soft:
            assert np.array_equal(np.isnan(soft), np.isnan(sp["p"])), f
            err = np.abs(soft[finite].astype(np.float64) - sp["p"][finite]).max()
            print("special values, %s: soft error %.3g (allowance %.3g)" % (f, err, allow))
            assert err <= allow, f
            assert (soft[finite][:, SP_HUGE] == 0.0).all(), f
        if form.q:
            assert np.array_equal(codes[keep], sp["drawn"][keep]), f
            assert codes[SP_NAN] == 0 and codes[SP_INF] == 0 and codes[SP_QZERO] == sp["qzero_code"], f
        else:
            assert np.array_equal(codes, sp["hard"]), f
            assert codes[SP_NAN] == 0 and codes[SP_EQUAL] == SP_DUP[0], f
    # every distance +inf (a token against codes of infinite norm only): index 0, a NaN row
    Einf = np.full((3, SP_D), 1e20, np.float32)
    soft, codes, dist = _run(dev, sp["x"][finite], Einf, SP_TEMP, FORMS["soft+dist"])
    assert (dist == np.inf).all() and not codes.any() and np.isnan(soft).all()
    _, drawn, _ = _run(dev, sp["x"][finite], Einf, SP_TEMP, FORMS["q"], np.ones((len(finite), 3), np.float32))
    assert not drawn.any()


@pytest.mark.gpu
def test_temperature_extremes(dev, oracle_mod):
    """one ordinary token, scaled by 8 so that every distance is above 34 and (-d) / 1e-37 overflows"""
    sp = _special(oracle_mod)
    x = np.float32(8.0) * sp["x"][SP_ORDINARY:SP_ORDINARY + 1]
    E = np.delete(sp["E"], SP_HUGE, axis=0)
    d = oracle_mod.token_distances(x[0], E)[None]
    K = E.shape[0]
    assert np.isfinite(d).all() and (d > 34.1).all()
    q = np.ones((1, K), np.float32)
    # every score overflows to -inf: the row maximum is -inf, s - max = NaN, as torch.softmax of the same scores gives
    assert np.isinf(R.scores(d, 1e-37)).all() and np.isnan(R.softmax64(d, 1e-37)).all()
    assert torch.isnan(torch.softmax(torch.from_numpy(R.scores(d, 1e-37)), dim=-1)).all()
    soft, codes, dist = _run(dev, x, E, 1e-37, FORMS["soft+dist"])
    assert np.array_equal(_bits(dist), _bits(d)) and np.isnan(soft).all() and codes[0] == np.argmin(d)
    assert _run(dev, x, E, 1e-37, FORMS["q"], q)[1][0] == 0
    # one-hot
    p = R.softmax64(d, 1e-6)
    assert sorted(p[0])[-2:] == [0.0, 1.0]
    soft, codes, _ = _run(dev, x, E, 1e-6, FORMS["soft+q"], q)
    assert np.array_equal(soft.astype(np.float64), p) and codes[0] == np.argmin(d)
    # uniform
    p = R.softmax64(d, 1e30)
    assert np.abs(p - 1.0 / K).max() <= 1e-20
    soft, codes, _ = _run(dev, x, E, 1e30, FORMS["soft+q"], q)
    assert (soft == soft[0, 0]).all() and abs(float(soft[0, 0]) - 1.0 / K) <= 4 * R.ulp32(1.0 / K) and codes[0] == 0


# ---- the other callers at D = 128 and a ragged K ----------------------------------------------------------------------------

@pytest.mark.gpu
def test_list_quantizer_at_d128(dev, oracle_mod):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2List
    c, inp = CASES["B"], _inputs("B", oracle_mod)
    m = VectorQuantize2List(c.K, c.D).to(dev).eval()
    m.codebook.weight.data[:-1].copy_(_t(dev)(inp["E"]))
    m.invalidate_codebook_cache()
    soft, code = m.get_soft_codes(_t(dev)(inp["x"]), temp=c.temp)
    _check_soft("list quantizer, case B", soft.cpu().numpy(), inp, c.K)
    assert np.array_equal(code.cpu().numpy(), inp["hard"])
    assert np.array_equal(_bits(soft.cpu().numpy()), _bits(_run(dev, inp["x"], inp["E"], c.temp, FORMS["soft"])[0]))


@pytest.mark.gpu
def test_rq_soft_codes_at_d128(dev, oracle_mod):
    from dynamicvectorquantization_amd.rq import RQBottleneck
    K, D, B, h, w, depth, temp = 67, 128, 2, 4, 4, 2, 8.0
    rq = RQBottleneck((h, w, D), (h, w, depth), K).to(dev).eval()
    books = []
    for i, cb in enumerate(rq.codebooks):
        Ei = synth.codebook_trained(K, D, seed=7701 + i) * np.float32(1.0 if i == 0 else 0.3)
        cb.weight.data[:-1].copy_(torch.from_numpy(Ei))
        cb.invalidate_codebook_cache()
        books.append(Ei)
    z = synth.z_tokens(books[0], B, h, w, 7711)
    xn = np.ascontiguousarray(z.transpose(0, 2, 3, 1))
    x = _t(dev)(xn)
    soft, hard = rq.get_soft_codes(x, temp=temp)
    N = B * h * w
    assert soft.shape == (B, h, w, depth, K) and hard.shape == (B, h, w, depth)
    ws = next(iter(rq._ws.values()))
    for i in range(depth):
        if i == 0:
            r = xn.reshape(N, D)
        else:
            off = _lib.lib.dvq_rq_residual_offset(N, D, depth, i)
            assert off > 0
            r = ws[off:off + N * D * 4].view(torch.float32).view(N, D).cpu().numpy()
            want = (xn.reshape(N, D) - books[0][hard[..., 0].reshape(N).cpu().numpy()]).astype(np.float32)
            assert np.array_equal(_bits(r), _bits(want))
        exp = _expected(oracle_mod, r, books[i], None, temp)
        exp["e_ref"], exp["allow"] = R.softmax32_error(exp["dist"], temp), R.soft_allowance(exp["dist"], temp)
        _check_soft("rq depth %d" % i, soft[..., i, :].reshape(N, K).cpu().numpy(), exp, K)
        assert np.array_equal(hard[..., i].reshape(N).cpu().numpy(), exp["hard"])
