"""The training-step kernels of csrc/ema_update.hip at the shapes and code skews they ship for.

`dvq_ema_accumulate_nchw_f32` picks one of three kernels.  The case table below was built for this dispatch predicate
(`dvq_launch_ema_accumulate`):

    sorted   ema_accumulate_sorted_kernel    K <= 4096 && HW % 4 == 0 && D % 16 == 0 && N >= 32 * EMS_BT   (EMS_BT = 2048: N >= 65536)
    combine  ema_accumulate_kernel<true>     otherwise, K <= 8192
    plain    ema_accumulate_kernel<false>    K > 8192

Every case names the form it is meant to hit in its id; `test_dispatch_predicate_is_the_one_the_case_table_was_built_for` finds
the predicate in the source and checks every id against it, so that a retuned threshold cannot quietly move the cases onto one form.

Two complementary checks run on every case:
  (a) exact: integer-valued latents in [-8, 8].  While 8 N < 2^24 every partial sum of every summation order is an exactly
      representable integer, so the sums are BIT-EQUAL to an int64 index_add_ and the counts equal bincount -- a dropped,
      duplicated or misrouted token in any 16-channel slice shows, whatever the skew;
  (b) rounding: normal latents against a float64 index_add_, per entry: |got[j, c] - S[j, c]| <= gamma_(n_j - 1) A[j, c] with
      A the same sum over |z|, gamma_m = m u / (1 - m u), u = 2^-24 -- the bound of ANY fp32 summation tree over n_j terms (the LDS
      partial sums and the float atomics are one); no constant of its own.  It implies that a row with n_j = 0 is exactly 0.0 and
      a row with n_j = 1 is bit-equal to its token.  It is loose for a hot code (n u = 1.5 % at n = 262144), which is why (a)
      exists; (b) shows that non-integer data takes the same route.
The references are torch / numpy / plain Python integers written here, never the code under test.

`dvq_restart_pick_i64` is deterministic and is restated in Python integers (splitmix64, multiply-high, first k distinct draws in
draw order); the kernel must equal the restatement bit for bit over a (k, n, seed) grid."""
import ctypes
import functools
import math
import os
import re
import zlib

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EUNSUPPORTED = -1, -2
EMS_BT, EMS_BC, EMS_LONG = 2048, 16, 128            # the sorted kernel's tile and its long-run threshold (pinned against the source below)
GUARD = 1024                                        # floats behind each output that must come back untouched
U32 = 2.0 ** -24                                    # unit roundoff of fp32


# ---------------------------------------------------------------------------------------------
# the dispatch predicate and the case table
# ---------------------------------------------------------------------------------------------
def _form(K, D, HW, N):
    if K <= 4096 and HW % 4 == 0 and D % 16 == 0 and N >= 32 * EMS_BT:
        return "sorted"
    return "combine" if K <= 8192 else "plain"


ALL_DISTS = ("uniform", "dual", "cubic", "hot10", "hot50", "one0", "oneK1", "run128_129", "long15", "runs1to9", "lastonly", "invalid5")

# (id prefix = the form it is meant to hit, B, D, HW, K, code distributions)
_SHAPES = (
    # sorted form
    ("sorted-production", 256, 256, 1024, 1024, ("uniform", "dual", "hot10", "oneK1")),     # 2048 items on 256 CUs: 8 per workgroup
    ("sorted-N65536", 64, 256, 1024, 1024, ("uniform",)),                                   # just over the threshold
    ("sorted-ragged36x36", 51, 64, 1296, 1024, ("uniform", "run128_129", "lastonly", "invalid5")),   # N = 66096 = 32 * 2048 + 560
    ("sorted-hw4", 16400, 32, 4, 512, ("uniform", "lastonly")),                             # a block spans 512 images; N % 2048 = 64
    ("sorted-hw64", 1025, 64, 64, 1024, ("cubic",)),                                        # a block spans 32 images; ragged
    ("sorted-D16", 64, 16, 1024, 1024, ("uniform", "hot50", "run128_129")),                 # one slice: the rotation degenerates
    ("sorted-D48", 192, 48, 1024, 1024, ALL_DISTS),                                         # 3 slices (5 = 2 mod 3); 288 items, 2 per workgroup:
                                                                                            # workgroups start inside a block and straddle two
    ("sorted-D80", 200, 80, 1024, 1024, ("uniform", "long15", "run128_129")),               # 5 slices (5 = 0 mod 5); 500 items, 2 per workgroup
    ("sorted-D64", 64, 64, 1024, 1024, ("uniform",)),
    ("sorted-D128", 64, 128, 1024, 1024, ("uniform", "cubic")),
    ("sorted-K4096", 64, 64, 1024, 4096, ("uniform", "cubic", "oneK1", "invalid5")),        # every scan thread owns four live entries
    ("sorted-K4093", 64, 32, 1024, 4093, ("uniform", "oneK1", "invalid5")),                 # K % 4 != 0: scan tail, k < K guards
    ("sorted-K5", 64, 32, 1024, 5, ("uniform", "one0", "oneK1", "run128_129", "invalid5")),
    # combine form: the same real shapes just outside each clause of the predicate
    ("combine-N65536-HW", 63, 256, 1024, 1024, ("uniform", "hot10")),
    ("combine-hw7x9", 1041, 64, 63, 1024, ("uniform", "cubic")),                            # N = 65583, HW % 4 != 0
    ("combine-hw31x33", 65, 32, 1023, 1024, ("uniform", "invalid5")),                       # N = 66495
    ("combine-D40", 64, 40, 1024, 1024, ("uniform",)),
    ("combine-D100", 64, 100, 1024, 1024, ("uniform", "hot50")),
    ("combine-K4097", 64, 16, 1024, 4097, ("uniform", "oneK1")),
    ("combine-K8192", 64, 16, 1024, 8192, ("uniform", "cubic", "oneK1")),
    ("combine-N35", 1, 24, 35, 64, ("uniform", "one0", "lastonly", "invalid5")),            # N < 64
    ("combine-N300", 3, 256, 100, 1024, ("uniform", "hot50")),                              # N % 64 != 0
    ("combine-N15360", 15, 64, 1024, 1024, ALL_DISTS),
    # plain form
    ("plain-K8193", 5, 64, 1023, 8193, ("uniform", "cubic", "hot50", "one0", "oneK1", "invalid5")),   # N = 5115: ragged
    ("plain-K16384", 5, 64, 1023, 16384, ("uniform", "cubic", "oneK1", "invalid5")),
)
CASES = [(name, B, D, HW, K, dist) for name, B, D, HW, K, dists in _SHAPES for dist in dists]
_case_ids = ["%s-%s" % (c[0], c[5]) for c in CASES]


def _seed(*parts):
    return zlib.crc32(repr(parts).encode())


def _invalid_values(K):
    return np.array([-1, K, K + 1, 2 ** 40, 2 ** 32, 2 ** 32 + 3, -(2 ** 40), np.iinfo(np.int64).min], dtype=np.int64)


def _plant(codes, block, runs, fill, rng):
    """token block `block` of the sorted kernel (EMS_BT tokens): exactly runs[c] tokens of code c at shuffled positions, the rest
    of the block drawn by fill(count) (codes that are not planted)"""
    lo, hi = block * EMS_BT, min((block + 1) * EMS_BT, codes.size)
    seq = np.concatenate([np.full(r, c, dtype=np.int64) for c, r in runs.items()])
    assert 0 <= lo < hi and seq.size <= hi - lo, "the shape is too small for this distribution"
    blk = np.concatenate([seq, np.asarray(fill(hi - lo - seq.size), dtype=np.int64)])
    codes[lo:hi] = rng.permutation(blk)


def make_codes(dist, B, HW, K, seed):
    """[B * HW] int64 codes on the host, from a seeded numpy generator"""
    rng = np.random.default_rng(seed)
    N = B * HW
    uni = rng.integers(0, K, N, dtype=np.int64)
    nblk = (N + EMS_BT - 1) // EMS_BT
    if dist == "uniform":
        return uni
    if dist == "dual":                                   # 2 x 2 copies of a coarse code on half the cells
        s = math.isqrt(HW)
        assert s * s == HW and s % 2 == 0
        up = lambda a: a.repeat(2, axis=1).repeat(2, axis=2)
        coarse = rng.integers(0, K, (B, s // 2, s // 2), dtype=np.int64)
        sel = rng.random((B, s // 2, s // 2)) < 0.5
        return np.where(up(sel), up(coarse), uni.reshape(B, s, s)).reshape(-1)
    if dist == "cubic":
        return np.minimum((K * rng.random(N) ** 3).astype(np.int64), K - 1)
    if dist in ("hot10", "hot50"):
        return np.where(rng.random(N) < (0.1 if dist == "hot10" else 0.5), np.int64(7 % K), uni)
    if dist == "one0":
        return np.zeros(N, dtype=np.int64)
    if dist == "oneK1":
        return np.full(N, K - 1, dtype=np.int64)
    if dist == "invalid5":
        return np.where(rng.random(N) < 0.05, rng.choice(_invalid_values(K), N), uni)
    if dist == "lastonly":                               # a block in which only the last token is valid: the first and the final one
        codes = uni.copy()
        first_end = min(EMS_BT, N)
        codes[:first_end] = -1
        codes[first_end - 1] = K // 2
        codes[(nblk - 1) * EMS_BT:] = -1
        codes[N - 1] = K - 1
        return codes
    codes = uni.copy()
    if dist == "run128_129":                             # both sides of the EMS_LONG boundary, in three blocks
        other = lambda n: rng.integers(2, K, n, dtype=np.int64)
        _plant(codes, 0, {0: EMS_LONG, 1: EMS_LONG + 1}, other, rng)
        _plant(codes, 1, {0: EMS_LONG + 1, 1: EMS_LONG}, other, rng)
        _plant(codes, nblk - 1, {0: EMS_LONG, 1: EMS_LONG + 1}, other, rng)      # (ragged where the shape is)
        return codes
    if dist == "long15":                                 # 15 long codes in one block: all that longk[] can hold
        other = lambda n: rng.integers(15, K, n, dtype=np.int64)
        _plant(codes, 0, {c: EMS_LONG + 1 for c in range(15)}, other, rng)                               # 1935 + 113 others
        _plant(codes, 1, {c: EMS_LONG + 1 if c < 14 else EMS_BT - 14 * (EMS_LONG + 1) for c in range(15)}, other, rng)   # nothing else
        return codes
    if dist == "runs1to9":                               # run lengths 1 .. 9: the left > 1 / 2 / 3 tails of the four-at-a-time walk
        planted = min(K - 1, 405)
        runs = {c: c % 9 + 1 for c in range(planted)}
        _plant(codes, 0, runs, lambda n: np.full(n, K - 1, dtype=np.int64), rng)
        _plant(codes, 2, runs, lambda n: np.full(n, K - 1, dtype=np.int64), rng)
        return codes
    raise ValueError(dist)


def _block_counts(codes, block, K):
    blk = codes[block * EMS_BT:(block + 1) * EMS_BT]
    return np.bincount(blk[(blk >= 0) & (blk < K)], minlength=K)


def test_dispatch_predicate_is_the_one_the_case_table_was_built_for():
    src = open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "ema_update.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    hint = " -- dvq_launch_ema_accumulate changed its dispatch: rebuild the case table _SHAPES of tests/test_ema_stats.py for the new predicate"
    for line in ("#define EMS_BT %d" % EMS_BT, "#define EMS_BC %d" % EMS_BC, "#define EMS_LONG %d" % EMS_LONG,
                 "if (K <= 4096 && (HW & 3) == 0 && (D & 15) == 0 && N >= 32 * EMS_BT) {",
                 "if (K <= 8192) hipLaunchKernelGGL(ema_accumulate_kernel<true>,",
                 "else hipLaunchKernelGGL(ema_accumulate_kernel<false>,",
                 "if (n0[u] > EMS_LONG)", "if (a[j] > EMS_LONG)"):
        assert line in flat, line + hint
    assert flat.count("dvq_launch_lds<ema_accumulate_sorted_kernel>") == 1, hint
    forms = {}
    for name, B, D, HW, K, dist in CASES:
        want = name.split("-")[0]
        assert _form(K, D, HW, B * HW) == want, (name, _form(K, D, HW, B * HW))
        assert 8 * B * HW < 2 ** 24, name
        forms.setdefault(want, set()).add(dist)
    assert set(forms) == {"sorted", "combine", "plain"}
    assert forms["sorted"] == set(ALL_DISTS) and forms["combine"] == set(ALL_DISTS)
    assert {"uniform", "hot50", "one0", "oneK1", "invalid5"} <= forms["plain"]
    assert len(set(_case_ids)) == len(_case_ids)


def test_code_distributions_hold_what_their_names_claim():
    """host-side: the planted blocks really hold runs of exactly 128 and 129, 15 long codes, run lengths 1 .. 9, a single valid
    token; the invalid codes include every kind"""
    B, HW, K = 51, 1296, 1024                            # ragged: 32 full blocks and one of 560 tokens
    N, last = B * HW, (B * HW - 1) // EMS_BT
    c = make_codes("run128_129", B, HW, K, 1)
    assert list(_block_counts(c, 0, K)[:2]) == [128, 129] and list(_block_counts(c, 1, K)[:2]) == [129, 128]
    assert list(_block_counts(c, last, K)[:2]) == [128, 129] and N - last * EMS_BT == 560
    c = make_codes("long15", B, HW, K, 2)
    for blk in (0, 1):
        n = _block_counts(c, blk, K)
        assert int((n > EMS_LONG).sum()) == 15 == EMS_BT // EMS_LONG - 1 and int((n[:15] > EMS_LONG).sum()) == 15
    assert _block_counts(c, 1, K)[15:].sum() == 0
    c = make_codes("runs1to9", B, HW, K, 3)
    n = _block_counts(c, 0, K)
    assert all(n[j] == j % 9 + 1 for j in range(405)) and n[K - 1] == EMS_BT - 2025
    c = make_codes("lastonly", B, HW, K, 4)
    assert _block_counts(c, 0, K).sum() == 1 and c[EMS_BT - 1] == K // 2 and _block_counts(c, last, K).sum() == 1 and c[N - 1] == K - 1
    c = make_codes("invalid5", B, HW, K, 5)
    bad = c[(c < 0) | (c >= K)]
    assert 0.03 * N < bad.size < 0.07 * N and set(bad.tolist()) == set(_invalid_values(K).tolist())
    for d in ("hot10", "hot50"):
        c = make_codes(d, B, HW, K, 6)
        assert abs((c == 7).mean() - (0.1 if d == "hot10" else 0.5)) < 0.01
    c = make_codes("dual", 4, 1024, K, 7).reshape(4, 16, 2, 16, 2)
    same = (c == c[:, :, :1, :, :1]).all(axis=(2, 4))
    assert 0.4 < same.mean() < 0.6
    c = make_codes("cubic", B, HW, K, 8)
    assert c.min() == 0 and c.max() == K - 1 and 0.45 < (c < K // 8).mean() < 0.55      # u^3 < 1/8: half the tokens
    assert make_codes("lastonly", 1, 35, 64, 9).tolist() == [-1] * 34 + [63]


# ---------------------------------------------------------------------------------------------
# dvq_ema_accumulate_nchw_f32
# ---------------------------------------------------------------------------------------------
def _accumulate(dev, z, codes, B, D, HW, K, cs_buf, vs_buf):
    from dynamicvectorquantization_amd import _lib
    assert z.is_contiguous() and codes.is_contiguous() and z.dtype == torch.float32 and codes.dtype == torch.int64
    assert z.numel() == B * D * HW and codes.numel() == B * HW and cs_buf.numel() == K + GUARD and vs_buf.numel() == K * D + GUARD
    with _lib.on_device(dev):
        _lib.check(_lib.lib.dvq_ema_accumulate_nchw_f32(z.data_ptr(), codes.data_ptr(), B, D, HW, K, cs_buf.data_ptr(),
                                                        vs_buf.data_ptr(), _lib.stream_ptr(dev)), "dvq_ema_accumulate_nchw_f32")
    torch.cuda.synchronize()


def _outputs(dev, K, D):
    """both outputs pre-filled with non-zero values (the header: both are overwritten), each with a trailing guard"""
    return torch.full((K + GUARD,), 3.5, device=dev), torch.full((K * D + GUARD,), -2.25, device=dev)


def _guards_intact(cs_buf, vs_buf, K, D):
    return bool((cs_buf[K:] == 3.5).all()) and bool((vs_buf[K * D:] == -2.25).all())


def _row_index(codes, K):
    """codes outside [0, K) are ignored: the reference sends them to a row K of its own, dropped afterwards"""
    return torch.where((codes >= 0) & (codes < K), codes, torch.full_like(codes, K))


def _tokens(z, B, D, HW, dtype):
    """[N, D] token matrix in `dtype`, one allocation"""
    return torch.empty((B, HW, D), dtype=dtype, device=z.device).copy_(z.view(B, D, HW).permute(0, 2, 1)).view(B * HW, D)


def _check_exact(dev, B, D, HW, K, codes, seed, bufs=None):
    N = B * HW
    assert 8 * N < 2 ** 24, "max|z| * N must stay below 2^24, or a partial sum may round and the check is void"
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randint(-8, 9, (B, D, HW), generator=g, device=dev).float()
    assert float(z.abs().max()) * N < 2 ** 24
    cs_buf, vs_buf = bufs if bufs is not None else _outputs(dev, K, D)
    _accumulate(dev, z, codes, B, D, HW, K, cs_buf, vs_buf)
    idx = _row_index(codes, K)
    ref_n = torch.bincount(idx, minlength=K + 1)[:K]
    ref = torch.zeros((K + 1, D), dtype=torch.int64, device=dev).index_add_(0, idx, _tokens(z, B, D, HW, torch.int64))[:K]
    assert int(ref.abs().max()) < 2 ** 24
    got_n, got = cs_buf[:K], vs_buf[:K * D].view(K, D)
    bad_n = (got_n != ref_n.float()).nonzero().flatten()
    assert bad_n.numel() == 0, "counts differ from bincount at %d codes, first %s: got %s, want %s" % (
        bad_n.numel(), bad_n[:5].tolist(), got_n[bad_n[:5]].tolist(), ref_n[bad_n[:5]].tolist())
    bad = (got != ref.float()).nonzero()                  # (integers below 2^24: the conversion is exact)
    assert bad.shape[0] == 0, "sums differ from the int64 index_add_ at %d entries of %d, first (code, channel) %s: got %s, want %s" % (
        bad.shape[0], K * D, bad[:5].tolist(), got[bad[:5, 0], bad[:5, 1]].tolist(), ref[bad[:5, 0], bad[:5, 1]].tolist())
    assert _guards_intact(cs_buf, vs_buf, K, D), "wrote behind cluster_size[K] or vectors_sum[K * D]"


def _check_rounding(dev, B, D, HW, K, codes, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    z = torch.randn((B, D, HW), generator=g, device=dev)
    cs_buf, vs_buf = _outputs(dev, K, D)
    _accumulate(dev, z, codes, B, D, HW, K, cs_buf, vs_buf)
    idx = _row_index(codes, K)
    n = torch.bincount(idx, minlength=K + 1)[:K]
    tok = _tokens(z, B, D, HW, torch.float64)
    del z
    S = torch.zeros((K + 1, D), dtype=torch.float64, device=dev).index_add_(0, idx, tok)[:K]
    A = torch.zeros((K + 1, D), dtype=torch.float64, device=dev).index_add_(0, idx, tok.abs_())[:K]
    del tok
    m = (n - 1).clamp(min=0).double() * U32               # gamma_(n - 1) in float64; 0 for n = 0 (the row is exactly 0.0) and for
    gamma = m / (1.0 - m)                                 # n = 1 (the row is bit-equal to its token)
    got = vs_buf[:K * D].view(K, D).double()
    assert torch.equal(cs_buf[:K].double(), n.double())
    err = (got - S).abs()
    over = (err > gamma[:, None] * A).nonzero()
    worst = float((err / (gamma[:, None] * A).clamp(min=1e-300)).max()) if bool((n > 1).any()) else 0.0
    print("max |got - S| / (gamma_(n-1) A) = %.3g" % worst)
    assert over.shape[0] == 0, "%d entries of %d outside gamma_(n-1) * sum|z|, first (code, channel) %s: got %s, want %s, n %s" % (
        over.shape[0], K * D, over[:5].tolist(), got[over[:5, 0], over[:5, 1]].tolist(), S[over[:5, 0], over[:5, 1]].tolist(),
        n[over[:5, 0]].tolist())
    assert _guards_intact(cs_buf, vs_buf, K, D), "wrote behind cluster_size[K] or vectors_sum[K * D]"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_ids)
def test_accumulate_integer_latents_are_summed_exactly(dev, case):
    """check (a) of the module docstring: bit-equal to an int64 index_add_, counts equal to bincount, guards untouched"""
    name, B, D, HW, K, dist = case
    codes = torch.from_numpy(make_codes(dist, B, HW, K, _seed(name, dist))).to(dev)
    _check_exact(dev, B, D, HW, K, codes, _seed(name, dist, "z-int"))
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=_case_ids)
def test_accumulate_real_latents_within_the_fp32_summation_bound(dev, case):
    """check (b) of the module docstring: per entry within gamma_(n_j - 1) * sum |z| of a float64 index_add_"""
    name, B, D, HW, K, dist = case
    codes = torch.from_numpy(make_codes(dist, B, HW, K, _seed(name, dist))).to(dev)
    _check_rounding(dev, B, D, HW, K, codes, _seed(name, dist, "z-real"))
    torch.cuda.empty_cache()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [("sorted", 192, 48, 1024, 1024), ("combine", 15, 64, 1024, 1024), ("plain", 5, 64, 1023, 8193)],
                         ids=lambda s: s[0])
def test_accumulate_overwrites_its_outputs(dev, shape):
    """two calls with different codes on the SAME output buffers: the second result owes nothing to the first"""
    form, B, D, HW, K = shape
    assert _form(K, D, HW, B * HW) == form
    bufs = _outputs(dev, K, D)
    for i, dist in enumerate(("hot50", "uniform", "oneK1")):
        codes = torch.from_numpy(make_codes(dist, B, HW, K, _seed(form, "twice", i))).to(dev)
        _check_exact(dev, B, D, HW, K, codes, _seed(form, "twice-z", i), bufs=bufs)


@pytest.mark.gpu
def test_train_forward_at_scale_runs_the_sorted_form_into_the_module_buffers(dev):
    """VectorQuantize2(K = 1024, D = 256).train() at B = 64, 32 x 32 (N = 65536: the sorted form) without restarts: cluster_size_ema,
    embed_ema and weight against the reference's expressions (quantize2_mask.py:89-115) as float64 torch ops on the codes the
    forward returned; the project's 1e-5 relative (include/dvq.h)"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    K, D, B, H, W = 1024, 256, 64, 32, 32
    assert _form(K, D, H * W, B * H * W) == "sorted"
    E = synth.codebook_trained(K, D, seed=7301)
    z = torch.from_numpy(synth.z_tokens(E, B, H, W, 7302)).to(dev)
    m = VectorQuantize2(K, D, restart_unused_codes=False).to(dev)
    m.codebook.weight.data[:-1].copy_(torch.from_numpy(E))
    m.codebook.embed_ema.copy_(torch.from_numpy(E))
    m.codebook.cluster_size_ema.copy_(torch.rand(K, generator=torch.Generator().manual_seed(7303)) * 100.0)
    cs0, emb0, pad0 = m.codebook.cluster_size_ema.double().clone(), m.codebook.embed_ema.double().clone(), m.codebook.weight.data[K].clone()
    decay, eps = float(m.codebook.decay), float(m.codebook.eps)
    m.train()
    _, _, (_, _, codes) = m(z)
    codes = codes.reshape(-1)
    assert int(codes.min()) >= 0 and int(codes.max()) < K
    n = torch.bincount(codes, minlength=K).double()
    S = torch.zeros((K, D), dtype=torch.float64, device=dev).index_add_(0, codes, _tokens(z, B, D, H * W, torch.float64))
    cs_r = cs0 * decay + (1 - decay) * n
    emb_r = emb0 * decay + (1 - decay) * S
    tot = cs_r.sum()
    w_r = emb_r / (tot * (cs_r + eps) / (tot + K * eps)).reshape(-1, 1)
    for name, got, ref in (("cluster_size_ema", m.codebook.cluster_size_ema, cs_r), ("embed_ema", m.codebook.embed_ema, emb_r),
                           ("weight", m.codebook.weight.data[:K], w_r)):
        err = float((got.double() - ref).abs().max() / ref.abs().max())
        print("%s: max |got - ref| / max |ref| = %.3g" % (name, err))
        assert err < 1e-5, (name, err)
    assert torch.equal(m.codebook.weight.data[K], pad0)          # the padding row is not touched


# ---------------------------------------------------------------------------------------------
# dvq_restart_pick_i64
# ---------------------------------------------------------------------------------------------
M64 = (1 << 64) - 1
PICK_K = (1, 2, 511, 1024, 1025, 1537, 2048)                     # draws per thread 1, 1, 1, 2, 3, 4, 4; table sizes 8 .. 16384
PICK_SEEDS = (0, M64, M64 - 4, 12345, 0x9E3779B97F4A7C15, 0xDEADBEEFCAFEF00D)     # (seed + i wraps around for the second and third)


def _pick_n(k):
    return (16 * k, 262144, 2 ** 32 - 1)                      # the smallest allowed, the production batch, the largest allowed


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


@functools.lru_cache(maxsize=None)
def restart_pick_restated(seed, n, k):
    """(the first k distinct values among the 2 k draws, in draw order; how many draws repeated an earlier one)"""
    draws = [(splitmix64((seed + i) & M64) * n) >> 64 for i in range(2 * k)]
    seen, out = set(), []
    for d in draws:
        if d not in seen:
            seen.add(d)
            out.append(d)
    return tuple(out[:k]), len(draws) - len(seen)


def test_restart_pick_restatement_checks_itself():
    """the generator against its published vectors; every draw inside [0, n); at n = 16 k the 2 k draws do repeat (the kernel's
    de-duplication has work to do) and still hold k distinct values (the 'slot keeps its own index' branch is unreachable)"""
    assert splitmix64(0) == 0xE220A8397B1DCDAF and splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert splitmix64(1234567) == 6457827717110365317 and splitmix64((1234567 + 0x9E3779B97F4A7C15) & M64) == 3203168211198807973
    assert [(2 * k + 1023) // 1024 for k in PICK_K] == [1, 1, 1, 2, 3, 4, 4]
    for k in PICK_K:
        for n in _pick_n(k):
            assert 16 * k <= n < 2 ** 32
            for seed in PICK_SEEDS:
                out, dup = restart_pick_restated(seed, n, k)
                assert len(out) == k and len(set(out)) == k and 0 <= min(out) and max(out) < n
                if n == 16 * k and k >= 511:
                    assert dup >= 1, (k, n, seed)          # about k / 8 expected


def test_restart_pick_refuses_what_the_header_excludes():
    """argument checks that need no device: 1 <= k <= 2048, 16 k <= n < 2^32, out not null"""
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    q = 256                                                   # a "pointer" that is never dereferenced: the refusal comes first
    assert L.dvq_restart_pick_i64(1, 16 * 100 - 1, 100, q, None) == EUNSUPPORTED and b"16 k <= n" in L.dvq_last_error_string()
    assert L.dvq_restart_pick_i64(1, 1 << 20, 0, q, None) == EUNSUPPORTED
    assert L.dvq_restart_pick_i64(1, 1 << 20, 2049, q, None) == EUNSUPPORTED
    assert L.dvq_restart_pick_i64(1, 2 ** 32, 1024, q, None) == EUNSUPPORTED
    assert L.dvq_restart_pick_i64(1, -1, 1, q, None) == EUNSUPPORTED
    assert L.dvq_restart_pick_i64(1, 1 << 20, 1024, None, None) == EINVAL and b"null" in L.dvq_last_error_string()
    assert L.dvq_restart_pick_i64.argtypes[0] is ctypes.c_uint64        # the whole 64-bit seed reaches the kernel


@pytest.mark.gpu
@pytest.mark.parametrize("k", PICK_K)
def test_restart_pick_equals_its_restatement(dev, k):
    """a pure function of (seed, n, k): bit-equal to the Python restatement, and the same on a second launch"""
    from dynamicvectorquantization_amd import _lib

    def launch(seed, n):
        out = torch.full((k + 8,), -7, dtype=torch.int64, device=dev)
        with _lib.on_device(dev):
            _lib.check(_lib.lib.dvq_restart_pick_i64(seed, n, k, out.data_ptr(), _lib.stream_ptr(dev)), "dvq_restart_pick_i64")
        torch.cuda.synchronize()
        assert bool((out[k:] == -7).all())
        return out[:k].cpu()

    for n in _pick_n(k):
        for seed in PICK_SEEDS:
            want, _ = restart_pick_restated(seed, n, k)
            got = launch(seed, n)
            assert torch.equal(got, torch.tensor(want, dtype=torch.int64)), (k, n, seed)
            assert torch.equal(launch(seed, n), got), (k, n, seed)
