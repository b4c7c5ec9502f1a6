"""The narrow widths (codebook_dim 3, 4, 8, 16): the exact assign kernel of csrc/vq_assign_narrow.hip, its C ABI
(dvq_vq_assign_narrow_*), the dispatch in quantize.vq_assign and the drop-in classes on top of it.

The contract is the wide kernels': codes and z_q bit for bit the reference's CPU path, the loss within 1e-5 relative
(_cases.loss_close).  The reference's outputs at these widths are the fixtures tests/golden/narrow_D*.npz
(tools/gen_golden_narrow.py, which also asserts that the oracle reproduces them: the pin); everything else is compared with
the oracle, with no token left out -- the kernel is exact.

Tolerances of the training tests: the straight-through gradient is one fused multiply-add chain per element in fp32 on both
sides, 1e-6 relative to the largest gradient; the EMA sums and the codebook gradient add up to 126 fp32 terms in an order of
their own (float atomics) -- 1e-5 relative per element, with 1e-5 of the largest element as the floor for entries whose
terms cancel."""
import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import synth
from tests._cases import GOLDEN, loss_close

WIDTHS = (4, 8, 16)
BETA = 0.25


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _golden(D):
    return np.load(os.path.join(GOLDEN, "narrow_D%d.npz" % D))


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_symbols_version_and_abi_validation_without_gpu():
    """the entry points are declared, exported and bound; validation needs no GPU (fake aligned "pointers": nothing is launched)"""
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    names = ("dvq_vq_assign_narrow_workspace_bytes", "dvq_vq_assign_narrow_nchw_f32", "dvq_vq_assign_narrow_flat_f32",
             "dvq_vq_assign_narrow_tile_codes")
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dvq.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert ("DVQ_API" in header and n + "(" in header), n
        assert hasattr(raw, n) and n in _lib.EXPORTS
    assert L.dvq_version() >= 1400
    EINVAL, EUNSUPPORTED = -1, -2
    a = 256                                                        # a "pointer" that passes the alignment checks

    def nchw(z=a, E=a, mask=0, B=2, D=4, HW=63, K=200, zq=a, codes=a, loss=0, ws=0, wsb=0):
        return L.dvq_vq_assign_narrow_nchw_f32(z, E, mask, B, D, HW, K, BETA, zq, codes, loss, ws, wsb, 0)

    def flat(z=a, E=a, mask=0, N=126, D=4, K=200, zq=a, codes=a, loss=0, ws=0, wsb=0):
        return L.dvq_vq_assign_narrow_flat_f32(z, E, mask, N, D, K, BETA, zq, codes, loss, ws, wsb, 0)

    for call in (nchw, flat):
        for null in ("z", "E", "codes"):
            assert call(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
        for D in (12, 32, 100, 3, 64, 256):
            assert call(D=D) == EUNSUPPORTED
            msg = L.dvq_last_error_string()
            assert b"4, 8 and 16" in msg and ("D=%d" % D).encode() in msg
        assert call(D=0) == EINVAL and call(K=0) == EINVAL and call(K=-5) == EINVAL
        assert call(K=1 << 20) == EUNSUPPORTED
        assert call(E=a + 8) == EINVAL                             # codebook rows are read with 16-byte loads
        need = L.dvq_vq_assign_narrow_workspace_bytes(126)
        assert need >= 8
        assert call(loss=a, ws=0, wsb=0) == EINVAL and b"workspace" in L.dvq_last_error_string()
        assert call(loss=a, ws=a, wsb=need - 1) == EINVAL and b"workspace" in L.dvq_last_error_string()
        assert call(loss=a, ws=a + 8, wsb=need) == EINVAL
    assert nchw(B=0) == EINVAL and nchw(HW=0) == EINVAL and flat(N=0) == EINVAL and flat(N=-1) == EINVAL
    assert nchw(B=1 << 16, HW=1 << 15) == EUNSUPPORTED and flat(N=1 << 31) == EUNSUPPORTED          # N < 2^31
    assert flat(z=a + 4) == EINVAL and flat(zq=a + 4) == EINVAL    # row-major rows: 16-byte accesses
    assert L.dvq_vq_assign_narrow_workspace_bytes(0) == 0 and L.dvq_vq_assign_narrow_workspace_bytes(-3) == 0
    assert L.dvq_vq_assign_narrow_workspace_bytes(1 << 20) >= 8 * ((1 << 20) // 256)
    for D in WIDTHS:
        t = L.dvq_vq_assign_narrow_tile_codes(D)
        assert t >= 64 and t % 4 == 0 and 2 * (t * D * 4 + t * 4) <= 160 * 1024      # two workgroups per CU fit the LDS
    assert L.dvq_vq_assign_narrow_tile_codes(12) == 0 and L.dvq_vq_assign_narrow_tile_codes(32) == 0


def test_dispatch_widths():
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import NARROW_WIDTHS, _padded_width, _wide_width
    assert NARROW_WIDTHS == WIDTHS
    assert [_padded_width(D) for D in (3, 4, 8, 16)] == [4, 4, 8, 16]
    assert [_padded_width(D) for D in (32, 64, 96, 128, 224, 256)] == [64, 64, 128, 128, 256, 256]      # as before
    for D in (12, 24, 48, 100, 512, 0, -4, 2, 5):
        with pytest.raises(_lib.DvqError, match="codebook_dim %d" % D):
            _padded_width(D)
    for D in (3, 4, 8, 16):
        with pytest.raises(_lib.DvqError, match="soft_assign: codebook_dim %d" % D):
            _wide_width(D, "soft_assign")
    assert _wide_width(32, "x") == 64 and _wide_width(256, "x") == 256


@pytest.mark.parametrize("D", (3, 4, 8, 16))
def test_goldens_match_the_oracle(D):
    """the pin, kept alive where the reference is absent: the oracle gives the reference's codes and z_q bit for bit"""
    oracle = _oracle()
    g = _golden(D)
    assert int(g["D"]) == D
    names = [str(n) for n in g["cases"]]
    assert names[:2] == ["trained", "ties"] and (("big" in names) == (D == 4))
    for name in names:
        z, E, mask = g[name + "_z"], g[name + "_E"], g[name + "_mask"]
        B = z.shape[0]
        for tag, m in (("vq2", mask), ("vqg", None)):
            o = oracle.vq_assign_nchw(z, E, m)
            assert np.array_equal(o["codes"], g[name + "_" + tag + "_codes"].reshape(B, -1))
            assert np.array_equal(_bits(o["zq"]), _bits(g[name + "_" + tag + "_zq"]))
            assert loss_close(oracle.vq_loss(o["sqerr"], o["numel"], BETA), g[name + "_" + tag + "_loss"])


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _call(form, z, E, mask=None, want_zq=True, want_loss=True):
    """the ABI entry point itself: z [B, D, HW] (form "nchw", HW = 1 included) or [N, D] ("flat"), GPU tensors"""
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    dev = z.device
    if form == "nchw":
        B, D, HW = z.shape
        N = B * HW
    else:
        N, D = z.shape
    K = E.shape[0]
    codes = torch.full((N,), -7, dtype=torch.int64, device=dev)
    zq = torch.full_like(z, float("nan")) if want_zq else None
    loss = torch.full((2,), float("nan"), device=dev) if want_loss else None
    ws = torch.empty(max(256, L.dvq_vq_assign_narrow_workspace_bytes(N)), dtype=torch.uint8, device=dev) if want_loss else None
    args = (_lib.ptr(zq), codes.data_ptr(), _lib.ptr(loss), _lib.ptr(ws), 0 if ws is None else ws.numel(), _lib.stream_ptr(dev))
    if form == "nchw":
        rc = L.dvq_vq_assign_narrow_nchw_f32(z.data_ptr(), E.data_ptr(), _lib.ptr(mask), B, D, HW, K, BETA, *args)
    else:
        rc = L.dvq_vq_assign_narrow_flat_f32(z.data_ptr(), E.data_ptr(), _lib.ptr(mask), N, D, K, BETA, *args)
    _lib.check(rc, "dvq_vq_assign_narrow_%s_f32" % form)
    torch.cuda.synchronize()
    return (codes.cpu().numpy(), None if zq is None else zq.cpu().numpy(), None if loss is None else loss.cpu().numpy())


def _rows(z):
    """[B, D, HW] -> the row-major tokens [B * HW, D] in the same token order"""
    return np.ascontiguousarray(z.transpose(0, 2, 1)).reshape(-1, z.shape[1])


def _check(form, dev, z, E, mask, ref, what):
    """both forms against ONE oracle result `ref` of z [B, D, HW]: codes and z_q bit-equal, every token; the loss 1e-5"""
    from oracle import oracle
    zin = z if form == "nchw" else _rows(z)
    codes, zq, loss = _call(form, _t(zin, dev), _t(E, dev), None if mask is None else _t(mask, dev))
    want_zq = ref["zq"] if form == "nchw" else _rows(ref["zq"])
    assert np.array_equal(codes, ref["codes"].reshape(-1)), what
    assert np.array_equal(_bits(zq), _bits(want_zq)), what
    ol = oracle.vq_loss(ref["sqerr"], ref["numel"], BETA)
    assert loss_close(loss[1], ol), (what, loss, ol)
    assert loss_close(loss[0], np.float32(ref["sqerr"] / ref["numel"])), what


@functools.lru_cache(maxsize=None)
def _edge_case(D, B, HW, K):
    oracle = _oracle()
    E = synth.codebook_trained(K, D, seed=7000 + D)
    z = synth.z_tokens(E, B, HW, 1, 7100 + 7 * D + HW + K % 97).reshape(B, D, HW)
    mask = np.where(synth.bernoulli(7200 + HW, (B, HW), 0.5), 1.0, 0.25).astype(np.float32)
    return z, E, mask, oracle.vq_assign_nchw(z, E, mask)


@pytest.mark.gpu
@pytest.mark.parametrize("D", (3, 4, 8, 16))
def test_goldens_on_the_device(dev, D):
    """every golden case through the two drop-in classes: the reference's codes, z_q (bits) and loss.  D = 3 runs at 4 with one
    zero channel; its loss is the mean over the 3 real channels"""
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantizer2
    g = _golden(D)
    for name in (str(n) for n in g["cases"]):
        z, E, mask = g[name + "_z"], g[name + "_E"], g[name + "_mask"]
        K = E.shape[0]
        with torch.no_grad():
            vq = VectorQuantize2(K, D, commitment_beta=BETA).to(dev).eval()
            vq.codebook.weight.data[:-1].copy_(_t(E, dev))
            xq, loss, (_, _, codes) = vq(_t(z, dev), codebook_mask=_t(mask, dev))
            assert np.array_equal(codes.cpu().numpy(), g[name + "_vq2_codes"]), name
            assert np.array_equal(_bits(xq.cpu().numpy()), _bits(g[name + "_vq2_zq"])), name
            assert loss_close(loss.item(), g[name + "_vq2_loss"]), (name, loss.item(), g[name + "_vq2_loss"])
            q = VectorQuantizer2(K, D, beta=BETA, legacy=False, sane_index_shape=True).to(dev).eval()
            q.embedding.weight.data.copy_(_t(E, dev))
            gq, gloss, (_, _, idx) = q(_t(z, dev))
            assert np.array_equal(idx.cpu().numpy(), g[name + "_vqg_codes"]), name
            assert np.array_equal(_bits(gq.cpu().numpy()), _bits(g[name + "_vqg_zq"])), name
            assert loss_close(gloss.item(), g[name + "_vqg_loss"]), name
            assert torch.equal(q.get_codebook_entry(idx.reshape(-1), None), q.embedding.weight[idx.reshape(-1)])
            assert torch.equal(vq.get_codebook_entry(codes), vq.codebook.weight[codes])


@pytest.mark.gpu
@pytest.mark.parametrize("form", ("nchw", "flat"))
@pytest.mark.parametrize("D", WIDTHS)
def test_shape_edges_against_the_oracle(dev, D, form):
    """B = 3 with HW = 1, 63, 65 (ragged last wave, odd and 4-byte-aligned planes), 131 (a second, ragged workgroup: 393 tokens of
    256 per workgroup) x K = 1, 200, one past a tile, one short of two tiles; K = 16384 at N = 128"""
    from dynamicvectorquantization_amd import _lib
    tile = _lib.lib.dvq_vq_assign_narrow_tile_codes(D)
    for HW in (1, 63, 65, 131):
        for K in (1, 200, tile + 1, 2 * tile - 1):
            z, E, mask, ref = _edge_case(D, 3, HW, K)
            _check(form, dev, z, E, mask, ref, (D, form, HW, K))
    z, E, mask, ref = _edge_case(D, 2, 64, 16384)
    _check(form, dev, z, E, mask, ref, (D, form, "K=16384"))


def _small_n():
    import re
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "dvq.h")).read()
    return int(re.search(r"#define\s+DVQ_NARROW_SMALL_N\s+(\d+)", header).group(1))


@pytest.mark.gpu
@pytest.mark.parametrize("D", WIDTHS)
def test_both_workgroup_shapes_at_their_threshold(dev, D):
    """up to DVQ_NARROW_SMALL_N tokens a workgroup is one wave of 64 tokens, above it two waves of 2 x 64 x 2: the last size of
    the first form (1024 workgroups) and a ragged size of the second (one valid token in the last workgroup, none in its second
    token slot), each with a tail tile; every token against the oracle"""
    from dynamicvectorquantization_amd import _lib
    tile = _lib.lib.dvq_vq_assign_narrow_tile_codes(D)
    small = _small_n()
    assert small % 256 == 0
    for N, K in ((small, 200), (small + 257, tile + 1)):
        z, E, mask, ref = _edge_case(D, 1, N, K)
        for form in ("nchw", "flat"):
            _check(form, dev, z, E, mask, ref, (D, form, N, K))
    z, E, mask, ref = _edge_case(D, 7, 9473, 3)                    # 66311 tokens in 7 odd planes: the second form across planes
    _check("nchw", dev, z, E, mask, ref, (D, "7 planes"))


@pytest.mark.gpu
def test_nchw_planes_at_odd_addresses_and_9x7(dev):
    """9 x 7 planes, B = 3, through vq_assign; and the same latents from a base pointer that is only 4-byte aligned"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign
    for D in WIDTHS:
        z, E, mask, ref = _edge_case(D, 3, 63, 200)
        zt = _t(z.reshape(3, D, 9, 7), dev)
        zq, codes, loss = vq_assign(zt, _t(E, dev), _CodebookPrep(), _t(mask, dev), beta=BETA)
        assert codes.shape == (3, 9, 7) and zq.shape == zt.shape
        assert np.array_equal(codes.cpu().numpy().reshape(3, -1), ref["codes"])
        assert np.array_equal(_bits(zq.cpu().numpy().reshape(3, D, 63)), _bits(ref["zq"]))
        big = torch.zeros(z.size + 3, device=dev)
        for shift in (1, 3):
            view = big[shift:shift + z.size].view(3, D, 63)
            view.copy_(_t(z, dev))
            assert view.data_ptr() % 16 != 0
            codes, zq, _ = _call("nchw", view, _t(E, dev), _t(mask, dev))
            assert np.array_equal(codes, ref["codes"].reshape(-1)) and np.array_equal(_bits(zq), _bits(ref["zq"]))


@pytest.mark.gpu
@pytest.mark.parametrize("D", WIDTHS)
def test_argmin_rules(dev, D):
    """duplicated rows (one pair across a tile boundary) give the lower index; NaN follows the oracle's take_min; the all-equal
    and the default-init (tie-stress) codebooks match the oracle"""
    from dynamicvectorquantization_amd import _lib
    oracle = _oracle()
    tile = _lib.lib.dvq_vq_assign_narrow_tile_codes(D)
    K = tile + 40
    E = synth.codebook_trained(K, D, seed=7300 + D)
    E[tile] = E[tile - 1]                                          # a pair straddling the tile boundary
    E[30] = E[5]
    E[tile + 20] = E[17]                                           # a pair two tiles apart
    z = synth.z_tokens(E, 1, 70, 1, 7310 + D).reshape(1, D, 70)
    z[0, :, 0], z[0, :, 1], z[0, :, 2] = E[tile], E[30], E[tile + 20]
    z[0, :, 3] = 2.0 * E[tile - 1]
    z[0, D - 1, 4] = np.nan                                        # a NaN latent: every distance NaN, index 0
    z[0, :, 5] = 0.0
    z[0, 0, 6] = np.inf
    for form in ("nchw", "flat"):
        ref = oracle.vq_assign_nchw(z, E, None)
        assert list(ref["codes"][0, :3]) == [tile - 1, 5, 17] and ref["codes"][0, 4] == 0
        _check(form, dev, z, E, None, ref, (D, form, "duplicates"))
        En = E.copy()
        En[tile + 3, 1] = np.nan                                   # a NaN code row is the minimum of every finite token
        En[9, 0] = np.nan                                          # ... and the FIRST NaN wins
        ref = oracle.vq_assign_nchw(z, En, None)
        assert ref["codes"][0, 7] == 9 and ref["codes"][0, 4] == 0
        _check(form, dev, z, En, None, ref, (D, form, "NaN code"))
        Ei = En.copy()
        Ei[9, 0] = 0.5
        Ei[0, :] = np.inf                                          # distance +inf at index 0, NaN further on
        _check(form, dev, z, Ei, None, oracle.vq_assign_nchw(z, Ei, None), (D, form, "inf code"))
        Eq = np.full((K, D), 0.25, np.float32)                     # all codes equal: index 0 everywhere
        ref = oracle.vq_assign_nchw(z[:, :, 8:], Eq, None)
        assert (ref["codes"] == 0).all()
        _check(form, dev, np.ascontiguousarray(z[:, :, 8:]), Eq, None, ref, (D, form, "all equal"))
        Ed = synth.codebook_default_init(K, D, seed=7320 + D)
        zs = np.ascontiguousarray(z[:, :, 8:]) * np.float32(0.002)
        _check(form, dev, zs, Ed, None, oracle.vq_assign_nchw(zs, Ed, None), (D, form, "default init"))


@pytest.mark.gpu
def test_optional_outputs_and_deterministic_loss(dev):
    for D in WIDTHS:
        z, E, mask, ref = _edge_case(D, 3, 131, 200)
        oracle = _oracle()
        for form in ("nchw", "flat"):
            zin = _t(z if form == "nchw" else _rows(z), dev)
            Et, mt = _t(E, dev), _t(mask, dev)
            full = _call(form, zin, Et, mt)
            again = _call(form, zin, Et, mt)
            assert np.array_equal(_bits(full[2]), _bits(again[2])), "the loss reduction is not deterministic"
            c1, zq1, l1 = _call(form, zin, Et, mt, want_zq=False)
            assert zq1 is None and np.array_equal(c1, full[0]) and np.array_equal(_bits(l1), _bits(full[2]))
            c2, zq2, l2 = _call(form, zin, Et, mt, want_loss=False)
            assert l2 is None and np.array_equal(c2, full[0]) and np.array_equal(_bits(zq2), _bits(full[1]))
            c3, zq3, l3 = _call(form, zin, Et, mt, want_zq=False, want_loss=False)
            assert zq3 is None and l3 is None and np.array_equal(c3, full[0])
            c4, zq4, l4 = _call(form, zin, Et, None)
            plain = oracle.vq_assign_nchw(z, E, None)
            assert np.array_equal(c4, full[0]) and np.array_equal(_bits(zq4), _bits(full[1]))
            assert loss_close(l4[1], oracle.vq_loss(plain["sqerr"], plain["numel"], BETA))
            assert loss_close(full[2][1], oracle.vq_loss(ref["sqerr"], ref["numel"], BETA))


@pytest.mark.gpu
def test_vq_assign_routes_by_layout_and_ignores_mode(dev):
    """vq_assign: [B, D, H, W] -> the NCHW form, [N, D] -> the flat form, any `mode`; the modules built on it"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantize2List, _CodebookPrep, vq_assign
    D = 8
    z, E, mask, ref = _edge_case(D, 3, 63, 200)
    prep = _CodebookPrep()
    for mode in (_lib.MODE_EXACT, _lib.MODE_FILTER):
        zq, codes, loss = vq_assign(_t(_rows(z), dev), _t(E, dev), prep, _t(mask, dev), beta=BETA, mode=mode)
        assert np.array_equal(codes.cpu().numpy(), ref["codes"].reshape(-1))
        assert np.array_equal(_bits(zq.cpu().numpy()), _bits(_rows(ref["zq"])))
    zq, codes, loss = vq_assign(torch.empty(0, D, 4, 4, device=dev), _t(E, dev), prep)
    assert codes.shape == (0, 4, 4) and torch.isnan(loss).all()
    with torch.no_grad():
        vq = VectorQuantize2(200, D, commitment_beta=BETA).to(dev).eval()
        vq.codebook.weight.data[:-1].copy_(_t(E, dev))
        emb, idx = vq.codebook(_t(_rows(z), dev))                  # VQEmbedding.forward / find_nearest_embedding
        assert np.array_equal(idx.cpu().numpy(), ref["codes"].reshape(-1))
        assert torch.equal(emb, vq.codebook.weight[idx])
        vl = VectorQuantize2List(200, D, commitment_beta=BETA).to(dev).eval()
        vl.codebook.weight.data[:-1].copy_(_t(E, dev))
        rows = _rows(z)
        items = [_t(rows[:50], dev), _t(rows[50:], dev)]
        xq_list, lloss, (_, _, code_list) = vl(items)
        assert np.array_equal(torch.cat(code_list).cpu().numpy(), ref["codes"].reshape(-1))
        assert np.array_equal(_bits(torch.cat(xq_list).cpu().numpy()), _bits(_rows(ref["zq"])))
        assert np.isfinite(lloss.item())


@pytest.mark.gpu
def test_vqgan_remap_and_index_shapes(dev, tmp_path):
    from dynamicvectorquantization_amd.quantize import VectorQuantizer2
    D, K = 4, 200
    g = _golden(D)
    z, E = g["trained_z"], g["trained_E"]
    used = np.arange(0, K, 2)
    np.save(str(tmp_path / "used.npy"), used)
    with torch.no_grad():
        for legacy in (True, False):
            q = VectorQuantizer2(K, D, beta=BETA, legacy=legacy).to(dev).eval()
            q.embedding.weight.data.copy_(_t(E, dev))
            zq, loss, (_, _, idx) = q(_t(z, dev))
            assert idx.shape == (z.shape[0] * 63,) and np.array_equal(idx.cpu().numpy(), g["trained_vqg_codes"].reshape(-1))
            assert loss_close(loss.item(), g["trained_vqg_loss"])
        q = VectorQuantizer2(K, D, beta=BETA, remap=str(tmp_path / "used.npy"), unknown_index=0, legacy=False).to(dev).eval()
        q.embedding.weight.data.copy_(_t(E, dev))
        _, _, (_, _, idx) = q(_t(z, dev))
        full = g["trained_vqg_codes"].reshape(-1)
        assert idx.shape == (full.size, 1)
        assert np.array_equal(idx.cpu().numpy().reshape(-1), np.where(full % 2 == 0, full // 2, 0))


@pytest.mark.gpu
def test_width_3_runs_padded_with_the_loss_rescaled(dev):
    from dynamicvectorquantization_amd.quantize import MaskVectorQuantize, _CodebookPrep, vq_assign
    oracle = _oracle()
    g = _golden(3)
    z, E, mask = g["trained_z"], g["trained_E"], g["trained_mask"]
    for zin, m in ((z, mask), (_rows(z.reshape(2, 3, 63)), mask.reshape(-1))):
        zq, codes, loss = vq_assign(_t(zin, dev), _t(E, dev), _CodebookPrep(), _t(m, dev), beta=BETA)
        o = oracle.vq_assign_nchw(z, E, mask)
        want = o["zq"] if zin.ndim == 4 else _rows(o["zq"].reshape(2, 3, 63))
        assert zq.shape == zin.shape and np.array_equal(_bits(zq.cpu().numpy()), _bits(want))
        assert np.array_equal(codes.cpu().numpy().reshape(-1), g["trained_vq2_codes"].reshape(-1))
        mean = np.float32(o["sqerr"] / o["numel"])                 # numel = N * 3: the mean over the REAL channels
        assert loss_close(loss[0].item(), mean) and loss_close(loss[1].item(), g["trained_vq2_loss"])
    with torch.no_grad():                                          # MaskVectorQuantize, L2, temp = 0, at 3 and 16 channels
        for D in (3, 16):
            gg = _golden(D)
            mq = MaskVectorQuantize(200, D).to(dev).eval()
            mq.embedding.weight.data.copy_(_t(gg["trained_E"], dev))
            mq.invalidate_codebook_cache()
            xq, _, (_, _, ind) = mq(_t(gg["trained_z"], dev), temp=0.)
            assert np.array_equal(ind.cpu().numpy().reshape(-1), gg["trained_vqg_codes"].reshape(-1))
            assert np.array_equal(_bits(xq.cpu().numpy()), _bits(gg["trained_vqg_zq"]))


def _close(got, want, rel):
    want = np.asarray(want, np.float64)
    return (np.abs(np.asarray(got, np.float64) - want) <= rel * np.maximum(np.abs(want), np.abs(want).max())).all()


@pytest.mark.gpu
@pytest.mark.parametrize("D", (4, 16))
def test_training_step_and_autograd(dev, D):
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantizer2
    g = _golden(D)
    z, E, mask = g["trained_z"], g["trained_E"], g["trained_mask"]
    B, K, numel = z.shape[0], E.shape[0], z.size
    wgt = synth.normal(7400 + D, z.shape)
    vq = VectorQuantize2(K, D, commitment_beta=BETA, restart_unused_codes=False).to(dev).train()
    with torch.no_grad():
        vq.codebook.weight.data[:-1].copy_(_t(E, dev))
        vq.codebook.embed_ema.copy_(_t(E, dev))
    x = _t(z, dev).requires_grad_(True)
    xq, loss, (_, _, codes) = vq(x, codebook_mask=_t(mask, dev))
    (3.0 * loss + (xq * _t(wgt, dev)).sum()).backward()
    c = codes.cpu().numpy().reshape(B, -1)
    assert np.array_equal(c, g["trained_vq2_codes"].reshape(B, -1))                 # the forward is the narrow kernel
    e = np.moveaxis(E[c], 2, 1).reshape(z.shape)
    want = wgt.astype(np.float64) + 3.0 * (BETA * 2.0 / numel) * (z.astype(np.float64) - e) * mask
    got = x.grad.cpu().numpy()
    assert np.isfinite(got).all() and (np.abs(got - want) <= 1e-6 * np.abs(want).max()).all()
    rows = _rows(z.reshape(B, D, -1)).astype(np.float64)
    counts = np.bincount(c.reshape(-1), minlength=K).astype(np.float64)
    sums = np.zeros((K, D))
    np.add.at(sums, c.reshape(-1), rows)
    assert _close(vq.codebook.cluster_size_ema.cpu().numpy(), 0.01 * counts, 1e-5)
    assert _close(vq.codebook.embed_ema.cpu().numpy(), 0.99 * E.astype(np.float64) + 0.01 * sums, 1e-5)
    assert torch.isfinite(vq.codebook.weight).all()

    q = VectorQuantizer2(K, D, beta=BETA, legacy=False).to(dev).train()
    with torch.no_grad():
        q.embedding.weight.copy_(_t(E, dev))
    x = _t(z, dev).requires_grad_(True)
    zq, loss, (_, _, idx) = q(x)
    (2.0 * loss).backward()
    ci = idx.cpu().numpy().reshape(-1)
    assert np.array_equal(ci, g["trained_vqg_codes"].reshape(-1))
    gw = np.zeros((K, D))
    np.add.at(gw, ci, 2.0 * (2.0 / numel) * (E[ci].astype(np.float64) - rows))
    assert _close(q.embedding.weight.grad.cpu().numpy(), gw, 1e-5)
    e = np.moveaxis(E[ci.reshape(B, -1)], 2, 1).reshape(z.shape)
    want = 2.0 * (BETA * 2.0 / numel) * (z.astype(np.float64) - e)
    assert (np.abs(x.grad.cpu().numpy() - want) <= 1e-6 * np.abs(want).max()).all()


@pytest.mark.gpu
def test_ops_without_a_narrow_kernel_still_raise(dev):
    """at 8 channels: the folded / fused quant_conv, the routed assign, RQBottleneck, get_soft_codes and the cosine quantizer
    raise DvqError naming the width.  (encode_* WITHOUT fold behind an 8-channel quant_conv is no fused path: select -> conv ->
    the narrow assign, which works.)"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.encode import encode_dual, encode_fixed
    from dynamicvectorquantization_amd.quantize import (MaskVectorQuantize, VectorQuantize2, _CodebookPrep, vq_assign,
                                                        vq_assign_routed_dual)
    from dynamicvectorquantization_amd.rq import RQBottleneck
    D, K = 8, 64
    vq = VectorQuantize2(K, D).to(dev).eval()
    conv = torch.nn.Conv2d(D, D, 1).to(dev).eval()
    hf, hc = torch.zeros(1, D, 8, 8, device=dev), torch.zeros(1, D, 4, 4, device=dev)
    ent = torch.zeros(1, 4, 4, device=dev)
    with torch.no_grad():
        with pytest.raises(_lib.DvqError, match="got 8"):
            encode_dual(None, vq, hf, hc, entropy=ent, quant_conv=conv, fold=True)
        with pytest.raises(_lib.DvqError, match="got 8"):
            encode_fixed(vq, hf, quant_conv=conv, fold=True)
        for kw in (dict(conv=conv), dict(conv=conv, fold=True, want_loss=False)):
            with pytest.raises(_lib.DvqError, match="got 8"):
                vq_assign(hf, vq.codebook.codes, _CodebookPrep(), **kw)
        with pytest.raises(_lib.DvqError, match="D=8"):
            vq_assign_routed_dual(hc, hf, vq.codebook.codes, _CodebookPrep(), entropy=ent, threshold=1.0)
        with pytest.raises(_lib.DvqError, match="codebook_dim 8"):
            RQBottleneck((8, 8, D), (8, 8, 2), K).to(dev).eval()(torch.zeros(1, 8, 8, D, device=dev))
        with pytest.raises(_lib.DvqError, match="codebook_dim 8"):
            vq.get_soft_codes(torch.zeros(1, 16, D, device=dev))
        with pytest.raises(_lib.DvqError, match="codebook_dim 8"):
            MaskVectorQuantize(K, D, use_cosine_sim=True).to(dev).eval()(hf)
        quant, emb_loss, info = encode_fixed(vq, hf, quant_conv=conv)          # the unfused order works
        assert quant.shape == hf.shape and torch.isfinite(emb_loss)
