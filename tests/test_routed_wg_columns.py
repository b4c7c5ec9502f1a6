"""The workgroup-wide column order of the LDS-staged routed pass 1 at D = 256 (csrc/dvq_pass1.h, WGC).
A workgroup is four image rows of 32 output positions, one per wave.  Its real columns (a position is real unless it is a copy:
not the first position of its cell) are ordered wave by wave, in column order; sorted position p is scored by wave p / 32 in MFMA
column group (p / 16) & 1, so the workgroup scores G = ceil(nreal_wg / 16) groups of its 8 and wave w runs the code loop on
clamp(ceil((nreal_wg - 32 w) / 16), 0, 2) of them: long, short, or not at all.  The B operands cross waves, and behind the loop
every position takes its cell owner's triple from a table indexed by sorted position.  Nothing the op returns may change: every
check is bit-exact against the CPU oracle's gate -> select -> assign (loss 1e-5) and against the per-lane form (SEL == 1: no
column order), which the op takes for branch tensors that are not 16-byte aligned.

nreal_wg, restated from the kernel.  Dual grid: the workgroup holds two cell rows of 16 cells, F of the 32 fine: 32 + 3 F (a
coarse cell has one real position, a fine cell's four positions are all real).  Triple grid: one cell row of 8 cells, c coarse,
m median, f fine: c + 4 m + 16 f = 8 + 3 (m + 5 f), so only counts of the form 8 + 3 j are reachable.

Shapes: every map is ONE workgroup; 36 of them, each laid out twice, fill B = 9 images of 32 x 32 (8 workgroups each): 72 token
blocks, which `pass1_plan` gives the staged form at K = 64 and at K = 1024 (`_form` of tests/test_routed_columns.py, asserted)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

from tests import test_routed_columns as RC

D, THR, KS = RC.D, RC.THR, RC.KS
B = 9


# ---- dual: which of a workgroup's 2 x 16 cells are fine ---------------------------------------------------------------------------
DUAL_F = (0, 5, 6, 10, 11, 16, 17, 21, 22, 26, 27, 32)            # G = 2, 3 | 4, 4 | 5, 5 | 6 (80 exactly | 83), 6 | 7, 7 | 8, 8
DUAL_PLACES = ("upper", "lower", "spread")


def _dual_wg(F, place, variant):
    """[2, 16] bool: F fine cells, all (or as many as fit) in the upper cell row, in the lower one, or spread over both; the
    second variant mirrors the cells left to right"""
    w = np.zeros((2, 16), bool)
    if place == "spread":
        up = (F + 1) // 2
        w[0, np.round(np.linspace(0, 15, up)).astype(int) if up else []] = True
        lo = F - up
        w[1, 15 - np.round(np.linspace(0, 15, lo)).astype(int) if lo else []] = True
    else:
        first = min(F, 16)
        r0, r1 = (0, 1) if place == "upper" else (1, 0)
        w[r0, :first] = True
        w[r1, 16 - (F - first):] = F > first
        if F == first:
            w[r1] = False
    if variant:
        w = w[:, ::-1]
    assert w.sum() == F, (F, place, variant, int(w.sum()))
    return np.ascontiguousarray(w)


def _dual_fine():
    """[9, 16, 16] bool and the (F, place) of every workgroup [9][8]"""
    cfgs = [(F, p) for F in DUAL_F for p in DUAL_PLACES]
    fine = np.zeros((B, 16, 16), bool)
    names = []
    for i in range(B * 8):
        F, p = cfgs[i % len(cfgs)]
        fine[i // 8, 2 * (i % 8):2 * (i % 8) + 2] = _dual_wg(F, p, i // len(cfgs))
        names.append((F, p))
    return fine, names


# ---- triple: grain per cell of a workgroup's 8 cells ------------------------------------------------------------------------------
def _triple_counts():
    """(c, m, f) per case: all coarse, the nearest reachable nreal_wg on both sides of every group boundary, no copies"""
    reach = {}
    for f in range(9):
        for m in range(9 - f):
            reach.setdefault(8 - m - f + 4 * m + 16 * f, []).append((8 - m - f, m, f))
    want = {8, 128}
    for b in range(16, 128, 16):
        want.add(max(n for n in reach if n <= b))
        want.add(min(n for n in reach if n > b))
    assert {8, 14, 17, 32, 35, 80, 83, 128} <= want
    out = []
    for n in sorted(want):
        out.extend(reach[n][:2])                                   # 32 is reachable as all median and as 4 + 3 median + 1 fine
    return out


def _triple_grains():
    """[9, 8, 8] grain per cell (0 coarse, 1 median, 2 fine) and the (c, m, f) of every workgroup: each case in four cell orders
    (fine cells left, right, spread, and a fixed shuffle)"""
    cfgs = _triple_counts()
    g = np.zeros((B, 8, 8), np.int64)
    names = []
    rng = np.random.RandomState(7)
    for i in range(B * 8):
        c, m, f = cfgs[i % len(cfgs)]
        row = np.array([2] * f + [1] * m + [0] * c, np.int64)
        v = i // len(cfgs)
        if v == 1:
            row = row[::-1]
        elif v == 2:
            row = np.concatenate([row[0::2], row[1::2][::-1]])
        elif v >= 3:
            row = row[rng.permutation(8)]
        g[i // 8, i % 8] = row
        names.append((c, m, f))
    return g, names


# ---- nreal_wg of a map, from the kernel's definition of a copy ---------------------------------------------------------------------
def _nreal_wg(rep):
    """rep [B, 32, 32]: positions per edge of the cell each output position belongs to -> real positions per workgroup [B, 8]"""
    y, x = np.mgrid[0:32, 0:32]
    real = (y % rep == 0) & (x % rep == 0)
    return real.reshape(rep.shape[0], 8, 4 * 32).sum(-1)


def test_maps_hit_the_stated_column_counts():
    """CPU: every map has the nreal_wg its name says, the dual ones cover G = 2 .. 8 with both sides of every boundary, the triple
    ones all coarse (one short wave, three without a group), 14 | 17, 32 | 35, the other boundaries and the map without copies"""
    fine, names = _dual_fine()
    rep = np.where(np.repeat(np.repeat(fine, 2, 1), 2, 2), 1, 2)
    n = _nreal_wg(rep).reshape(-1)
    assert [int(v) for v in n] == [32 + 3 * F for F, _ in names]
    G = -(-n // 16)
    assert sorted(set(G)) == [2, 3, 4, 5, 6, 7, 8] and {80, 83} <= set(n)
    assert {(F, p) for F, p in names} == {(F, p) for F in DUAL_F for p in DUAL_PLACES}
    reach = [32 + 3 * F for F in range(33)]
    for b in range(48, 128, 16):                                   # the nearest reachable counts on both sides of a boundary
        assert max(v for v in reach if v <= b) in n and min(v for v in reach if v > b) in n, b
    g, tn = _triple_grains()
    rep3 = np.repeat(np.repeat(np.array([4, 2, 1])[g], 4, 1), 4, 2)
    n3 = _nreal_wg(rep3).reshape(-1)
    assert [int(v) for v in n3] == [c + 4 * m + 16 * f for c, m, f in tn]
    assert {8, 14, 17, 32, 35, 47, 50, 62, 65, 80, 83, 92, 98, 104, 113, 128} == set(int(v) for v in n3)
    assert (8, 0, 0) in tn and (0, 0, 8) in tn and (0, 8, 0) in tn and (4, 3, 1) in tn
    assert sorted(set(-(-n3 // 16))) == [1, 2, 3, 4, 5, 6, 7, 8]


def test_headline_column_groups_are_the_counted_ones():
    """CPU: tools/short_wave_share.py on the headline's own inputs: 6144 workgroups, 6.81 column groups per workgroup under the
    per-wave rule, 6.00 packed per row pair, 5.43 packed per workgroup, and the histogram of G"""
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "short_wave_share.py")
    spec = importlib.util.spec_from_file_location("short_wave_share", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    t = mod.column_groups(np.concatenate(mod.headline_fine_cells(), 0))
    assert t["workgroups"] == 6144
    assert round(t["per_wave"], 2) == 6.81 and round(t["per_row_pair"], 2) == 6.00 and round(t["per_workgroup"], 2) == 5.43
    assert t["histogram"] == {"4": 126, "5": 3398, "6": 2470, "7": 148, "8": 2}
    # the rules on a hand-made pair of workgroups: all coarse (16, 0, 16, 0 real columns), and 5 + 0 fine cells (21, 10, 16, 0)
    t2 = mod.column_groups(np.array([[0, 0], [5, 0]]))
    assert (t2["per_wave"], t2["per_row_pair"], t2["per_workgroup"]) == ((4 + 5) / 2, (2 + 3) / 2, (2 + 3) / 2)


# ---- GPU ----------------------------------------------------------------------------------------------------------------------
_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _dual_inputs(K, tie):
    def make():
        from dynamicvectorquantization_amd import synth
        E = RC._tie_codebook(K) if tie else RC._codebook(K)
        hc = synth.z_tokens(E, B, 16, 16, 5100 + K)
        hf = synth.z_tokens(E, B, 32, 32, 5200 + K)
        return E, hc, hf, RC._entropy(_dual_fine()[0])
    return _memo(("dual", K, tie), make)


def _run_dual(dev, oracle_mod, K, sl, tie=False):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_dual
    E, hc, hf, ent = _dual_inputs(K, tie)
    nb = sl.stop - sl.start
    assert RC._form(nb, K) == "staged" and RC._form(nb, K, aligned=False) == "per-lane"
    og = oracle_mod.entropy_gate(ent[sl], THR)
    o_sel = oracle_mod.route_select_dual(og, hc[sl], hf[sl])
    o = oracle_mod.vq_assign_nchw(o_sel["h_dual"], E, o_sel["codebook_mask"])
    t = RC._t(dev)
    tE, te = t(E), t(ent[sl])
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    with torch.no_grad():
        r2 = vq_assign_routed_dual(t(hc[sl]), t(hf[sl]), tE, p2, entropy=te, threshold=THR)
        f2 = p2.fallback_count()
        r1 = vq_assign_routed_dual(RC._off(hc[sl], dev), RC._off(hf[sl], dev), tE, p1, entropy=te, threshold=THR)
        f1 = p1.fallback_count()
    RC._check(r2, og, o_sel, o, oracle_mod)
    RC._check(r1, og, o_sel, o, oracle_mod)
    RC._same_bits(r2, r1)
    return f2, f1


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_dual_fine_cells_per_workgroup(dev, oracle_mod, K):
    """F = 0 .. 32 fine cells in a workgroup's two cell rows, upper / lower / spread: columns imported from every other wave,
    waves with two, one and no column group in one workgroup, 80 real columns exactly, the identity order"""
    f2, f1 = _run_dual(dev, oracle_mod, K, slice(0, B))
    assert f2 == f1, (f2, f1)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_triple_counts_at_every_group_boundary(dev, oracle_mod, K):
    """nreal_wg = c + 4 m + 16 f from 8 (all coarse) to 128 (no copies), on both sides of every group boundary"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_triple
    assert RC._form(B, K) == "staged" and RC._form(B, K, aligned=False) == "per-lane"
    E = RC._codebook(K)
    g, _ = _triple_grains()
    logits = synth.normal(5700 + K, (B, 8, 8, 3), 0.0, 1.0).astype(np.float32)
    np.put_along_axis(logits, g[..., None], np.float32(9.0), -1)    # the wanted grain wins by a wide margin
    br = [synth.z_tokens(E, B, 8 << k, 8 << k, 5300 + K + k) for k in range(3)]
    o_sel = oracle_mod.route_select_triple(logits, br[0], br[1], br[2])
    assert np.array_equal(o_sel["indices"], g)
    o = oracle_mod.vq_assign_nchw(o_sel["h_triple"], E, o_sel["codebook_mask"])
    t = RC._t(dev)
    tE, tl = t(E), t(logits)
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    with torch.no_grad():
        r2 = vq_assign_routed_triple(t(br[0]), t(br[1]), t(br[2]), tE, p2, tl)
        f2 = p2.fallback_count()
        r1 = vq_assign_routed_triple(RC._off(br[0], dev), RC._off(br[1], dev), RC._off(br[2], dev), tE, p1, tl)
        f1 = p1.fallback_count()
    RC._check(r2, None, o_sel, o, oracle_mod)
    RC._check(r1, None, o_sel, o, oracle_mod)
    RC._same_bits(r2, r1)
    assert f2 == f1, (f2, f1)


@pytest.mark.gpu
def test_tie_codebook_sends_every_owner_to_the_resolver(dev, oracle_mod):
    """the tie-stress codebook of tests/test_routed_copies.py on three of the images (24 of the maps, every F and every placement
    among them): every token's two best scores tie, so every cell's owner is undecided, queues a record, and the resolver corrects
    all of its copies; the codes must be the oracle's.  A workgroup with more than 64 owners fills its shard and WHICH owners are
    listed instead is the order the waves draw their slots in, so only the number queued is compared between the forms.
    K = 64: staged at B = 3."""
    for b0 in (0, 3, 6):
        f2, f1 = _run_dual(dev, oracle_mod, 64, slice(b0, b0 + 3), tie=True)
        assert f2[0] > 0 and f1[0] == f2[0], (b0, f2, f1)
