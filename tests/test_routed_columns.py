"""The column order and the short code loop of the LDS-staged routed pass 1 (csrc/dvq_pass1.h, SEL == 2).
A wave is one image row of 32 output positions in two MFMA column groups of 16.  It sorts its real columns in front of the copies
of coarser cells, and with at most 16 real columns (`nreal <= 16`) it runs the code loop on the first group alone.  Nothing the op
returns may change: every check is bit-exact against the CPU oracle's gate -> select -> assign (loss 1e-5) and against the
per-lane form (SEL == 1: no column order, no short loop), which the op takes for branch tensors that are not 16-byte aligned.

What a row's `nreal` is, restated from the kernel: a position is real unless it is a copy (not the first position of its cell).
Dual grid, f fine cells of 16 in the cell row: the even image row has 16 + f real columns (every cell's first position, and the
fine cells' second), the odd row 2 f.  Triple grid, cell row of 8 cells with c coarse, m median, f fine: row 0 has c + 2 m + 4 f,
row 2 has 2 m + 4 f, rows 1 and 3 have 4 f.

Shapes: B = 2 on a 32 x 32 grid has both row parities in every workgroup (four rows) and two workgroups per pair of cell rows.
That is 16 token blocks: `pass1_plan` (csrc/vq_assign_filter.hip) gives the staged form from 65 blocks on, and below that whenever
the small-batch split declines -- K = 64 leaves a slice fewer than two code tiles, so B = 2 is staged there; at K = 1024 the split
form (per-lane select) serves B = 2.  The cases therefore run twice: each alone at B = 2 with both codebooks, and all of them
as ONE batch (B = 16 dual, B = 10 triple: 128 / 80 blocks), which is staged at K = 1024 too.  `_form` restates the plan and every
test asserts the form it means to exercise."""
import numpy as np
import pytest
import torch

from tests import _cases as C

D = 256
THR = 1.6777750253677368                                           # the benchmark's entropy threshold; any value serves
KS = (64, 1024)


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _off(a, dev):
    """the array as a contiguous device view 4 bytes into its storage: not 16-byte aligned -> per-lane select"""
    a = np.ascontiguousarray(a)
    buf = torch.empty(a.size + 1, dtype=torch.float32, device=dev)
    v = buf[1:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


def _form(B, K, aligned=True):
    """pass1_plan for a routed op without conv on a 32 x 32 output grid"""
    nb = B * 8
    tiles = (K + 31) // 32
    ks = 1
    if nb <= 64:                                                  # DVQ_SPLIT_MAX_BLOCKS
        ks = 8                                                    # DVQ_SPLIT_MAX_SLICES
        while ks > 1 and (nb * ks > 256 or tiles // ks < 2):
            ks >>= 1
    if ks > 1:
        return "split"
    return "staged" if aligned else "per-lane"


# ---- dual: which of the 16 cells of a cell row are fine, per case: [2 images][16 cell rows][16 cells] ----------------------------
def _row(cells):
    r = np.zeros(16, bool)
    r[list(cells)] = True
    return r


def _dual_cases():
    none, full = _row([]), _row(range(16))
    spread8 = [_row(range(k % 2, 16, 2)[:8]) if k % 3 else _row([0, 1, 4, 5, 8, 9, 12, 13]) for k in range(16)]     # exactly 8
    spread9 = [_row(list(range(k % 2, 16, 2)) + [(2 * k + 1 - k % 2) % 16]) for k in range(16)]                     # exactly 9
    left = [_row(range(1 + k % 8)) for k in range(16)]            # 1 .. 8 fine cells, all in the left half
    right = [_row(range(16 - (1 + k % 8), 16)) for k in range(16)]  # ... all in the right half: real columns only in group 1
    checker = [_row(range(k % 2, 16, 2)) for k in range(16)]
    cases = {
        "none_fine": [[none] * 16] * 2,
        "all_fine": [[full] * 16] * 2,
        "boundary_8": [spread8, spread8[::-1]],
        "boundary_9": [spread9, spread9[::-1]],
        "left_block": [left, left[::-1]],
        "right_block": [right, right[::-1]],
        "checkerboard": [checker, checker[::-1]],
        # cell rows alternate all coarse / all fine: a workgroup (two cell rows) holds short and long waves
        "mixed_row_pairs": [[none if k % 2 == 0 else full for k in range(16)], [full if k % 2 == 0 else none for k in range(16)]],
    }
    out = {}
    for name, imgs in cases.items():
        out[name] = np.stack([np.stack(rows) for rows in imgs])   # [2, 16, 16] bool
    for r in out["boundary_8"].reshape(-1, 16):
        assert r.sum() == 8
    for r in out["boundary_9"].reshape(-1, 16):
        assert r.sum() == 9
    assert all(not r[8:].any() and r.any() for r in out["left_block"].reshape(-1, 16))
    assert all(not r[:8].any() and r.any() for r in out["right_block"].reshape(-1, 16))
    return out


DUAL = _dual_cases()
DUAL_NAMES = list(DUAL)


def _dual_nreal(fine):
    """real columns of the even and the odd image row of every cell row: [..., 2]"""
    f = fine.sum(-1)
    return np.stack([16 + f, 2 * f], -1)


def test_dual_maps_hit_the_edges_of_the_rule():
    """CPU: the hand-made maps hold what their names say, in terms of the kernel's nreal"""
    n = {k: _dual_nreal(v) for k, v in DUAL.items()}
    assert np.all(n["none_fine"] == [16, 0])                      # every row short, the odd ones with no real column
    assert np.all(n["all_fine"] == 32)                            # no copies: identity order
    assert np.all(n["boundary_8"][..., 1] == 16) and np.all(n["boundary_9"][..., 1] == 18)
    assert np.all(n["boundary_8"][..., 0] == 24) and np.all(n["boundary_9"][..., 0] == 25)
    assert n["left_block"][..., 1].max() == 16 and n["left_block"][..., 1].min() == 2
    assert set(np.unique(n["mixed_row_pairs"][..., 1])) == {0, 32}
    # boundary + 1 in the kernel's own terms (17 real columns) exists only on even rows of a dual grid (16 + f) and is part of
    # the left / right blocks (f = 1); the triple case below has odd rows at exactly 16 and 20
    assert (n["left_block"][..., 0] == 17).any() and (n["right_block"][..., 0] == 17).any()


def _entropy(fine):
    return np.where(fine, np.float32(THR + 1.0), np.float32(THR - 1.0)).astype(np.float32)


def _codebook(K):
    from dynamicvectorquantization_amd import synth
    E = synth.codebook_trained(K, D, seed=91)
    E[7] = E[3]                                                   # duplicate code: the first index wins
    return E


def _tie_codebook(K):
    """the tie-stress codebook of tests/test_routed_copies.py: default-initialised, second half = first half, so every token's best
    and second-best score are equal and every cell's owner is undecided"""
    from dynamicvectorquantization_amd import synth
    E = synth.codebook_default_init(K, D)
    E[K // 2:] = E[:K // 2]
    return E


_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _dual_inputs(K, tie=False):
    """(E, h_coarse [16, D, 16, 16], h_fine [16, D, 32, 32], entropy [16, 16, 16]): the eight cases, two images each"""
    def make():
        from dynamicvectorquantization_amd import synth
        E = _tie_codebook(K) if tie else _codebook(K)
        B = 2 * len(DUAL_NAMES)
        hc = synth.z_tokens(E, B, 16, 16, 4100 + K)
        hf = synth.z_tokens(E, B, 32, 32, 4200 + K)
        ent = np.concatenate([_entropy(DUAL[n]) for n in DUAL_NAMES], 0)
        return E, hc, hf, ent
    return _memo(("dual", K, tie), make)


def _dual_oracle(oracle_mod, K, sl, tie=False):
    def make():
        E, hc, hf, ent = _dual_inputs(K, tie)
        og = oracle_mod.entropy_gate(ent[sl], THR)
        o_sel = oracle_mod.route_select_dual(og, hc[sl], hf[sl])
        return og, o_sel, oracle_mod.vq_assign_nchw(o_sel["h_dual"], E, o_sel["codebook_mask"])
    return _memo(("dual_oracle", K, sl.start, sl.stop, tie), make)


def _check(r, og, o_sel, o, oracle_mod):
    B = o["codes"].shape[0]
    if og is not None:
        assert np.array_equal(r["gate"].cpu().numpy(), og), "gate"
    assert np.array_equal(r["indices"].cpu().numpy(), o_sel["indices"]), "grain indices"
    assert np.array_equal(r["codebook_mask"].cpu().numpy(), o_sel["codebook_mask"]), "codebook_mask"
    assert np.array_equal(r["codes"].cpu().numpy().reshape(B, -1), o["codes"]), "codes"
    assert np.array_equal(r["zq"].cpu().numpy().view(np.int32), o["zq"].view(np.int32)), "z_q"
    assert C.loss_close(float(r["loss"][1]), oracle_mod.vq_loss(o["sqerr"], o["numel"], 0.25)), "loss"


def _same_bits(a, b):
    """codes, z_q and loss of the staged form equal the per-lane form's bit for bit"""
    assert torch.equal(a["codes"], b["codes"]), "codes vs per-lane"
    assert torch.equal(a["zq"].view(torch.int32), b["zq"].view(torch.int32)), "z_q vs per-lane"
    assert torch.equal(a["loss"].view(torch.int32), b["loss"].view(torch.int32)), "loss vs per-lane"


def _run_dual(dev, oracle_mod, K, sl, expect, tie=False):
    """the op on aligned tensors and on offset views (per-lane select), each against the oracle and against each other
    -> the two fallback counts (queued, listed)"""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_dual
    E, hc, hf, ent = _dual_inputs(K, tie)
    B = sl.stop - sl.start
    assert _form(B, K) == expect and _form(B, K, aligned=False) in ("per-lane", "split")
    og, o_sel, o = _dual_oracle(oracle_mod, K, sl, tie)
    t = _t(dev)
    tE, te = t(E), t(ent[sl])
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    with torch.no_grad():
        r2 = vq_assign_routed_dual(t(hc[sl]), t(hf[sl]), tE, p2, entropy=te, threshold=THR)
        f2 = p2.fallback_count()
        r1 = vq_assign_routed_dual(_off(hc[sl], dev), _off(hf[sl], dev), tE, p1, entropy=te, threshold=THR)
        f1 = p1.fallback_count()
    _check(r2, og, o_sel, o, oracle_mod)
    _check(r1, og, o_sel, o, oracle_mod)
    _same_bits(r2, r1)
    return f2, f1


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("case", DUAL_NAMES)
def test_dual_case_alone(dev, oracle_mod, case, K):
    """each map at B = 2: staged at K = 64; at K = 1024 the small-batch split form serves the shape (see the module text)"""
    i = DUAL_NAMES.index(case)
    f2, f1 = _run_dual(dev, oracle_mod, K, slice(2 * i, 2 * i + 2), "staged" if K == 64 else "split")
    assert f2 == f1, (f2, f1)


@pytest.mark.gpu
@pytest.mark.parametrize("K", KS)
def test_dual_cases_as_one_batch(dev, oracle_mod, K):
    """all eight maps as one batch of 16 images: the staged form at both codebook sizes, per-tile seeds never (K <= 1024)"""
    f2, f1 = _run_dual(dev, oracle_mod, K, slice(0, 16), "staged")
    assert f2 == f1, (f2, f1)


# ---- triple: logits per 4 x 4 cell row of 8 cells --------------------------------------------------------------------------------
def _triple_grains():
    """grain per cell [10, 8, 8] (0 coarse, 1 median, 2 fine).  Images 0 / 1: cell rows all coarse, all median, all fine, and the
    mix with exactly 16 real columns in image row 1 (4 fine cells), at every position of the cell-row cycle and in both workgroup
    halves; images 2 .. 9: the same rows cycled, the mix with its fine cells left / right / spread and 5 fine cells (20 columns)"""
    rows = [np.zeros(8, np.int64), np.ones(8, np.int64), np.full(8, 2, np.int64),
            np.array([2, 0, 1, 2, 0, 2, 1, 2], np.int64),          # 4 fine: rows 1 and 3 have 16 real columns, row 0: 2 + 4 + 16
            np.array([2, 2, 2, 2, 0, 1, 0, 1], np.int64),          # 4 fine, left
            np.array([1, 0, 0, 1, 2, 2, 2, 2], np.int64),          # 4 fine, right: every real column of row 1 from group 1
            np.array([2, 2, 0, 2, 1, 2, 0, 2], np.int64),          # 5 fine: 20 real columns, long
            np.array([0, 1, 0, 1, 0, 1, 0, 1], np.int64)]          # no fine: row 0 has 12, row 2 has 8, rows 1 and 3 none
    g = np.empty((10, 8, 8), np.int64)
    for b in range(10):
        for y in range(8):
            g[b, y] = rows[(y + 3 * b) % len(rows)]
    assert all((g[0, y] == 2).sum() in (0, 4, 5, 8) for y in range(8)) and ((g[0] == 2).sum(-1) == 4).any()
    return g


def _triple_inputs(K):
    def make():
        from dynamicvectorquantization_amd import synth
        E = _codebook(K)
        g = _triple_grains()
        B = g.shape[0]
        logits = synth.normal(4700 + K, (B, 8, 8, 3), 0.0, 1.0).astype(np.float32)
        np.put_along_axis(logits, g[..., None], np.float32(9.0), -1)            # the wanted grain wins by a wide margin
        br = [synth.z_tokens(E, B, 8 << k, 8 << k, 4300 + K + k) for k in range(3)]
        return E, br, logits, g
    return _memo(("triple", K), make)


@pytest.mark.gpu
@pytest.mark.parametrize("K,B", [(64, 2), (64, 10), (1024, 2), (1024, 10)])
def test_triple_logits_all_of_one_grain_and_the_16_column_mix(dev, oracle_mod, K, B):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_triple
    E, br, logits, g = _triple_inputs(K)
    assert _form(B, K) == ("split" if (K, B) == (1024, 2) else "staged")
    br = [a[:B] for a in br]
    o_sel = oracle_mod.route_select_triple(logits[:B], br[0], br[1], br[2])
    assert np.array_equal(o_sel["indices"], g[:B])                # the crafted logits give the crafted grains
    o = oracle_mod.vq_assign_nchw(o_sel["h_triple"], E, o_sel["codebook_mask"])
    t = _t(dev)
    tE, tl = t(E), t(logits[:B])
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    with torch.no_grad():
        r2 = vq_assign_routed_triple(t(br[0]), t(br[1]), t(br[2]), tE, p2, tl)
        f2 = p2.fallback_count()
        r1 = vq_assign_routed_triple(_off(br[0], dev), _off(br[1], dev), _off(br[2], dev), tE, p1, tl)
        f1 = p1.fallback_count()
    _check(r2, None, o_sel, o, oracle_mod)
    _check(r1, None, o_sel, o, oracle_mod)
    _same_bits(r2, r1)
    assert f2 == f1, (f2, f1)


# ---- the rare branches: undecided cells of short waves ---------------------------------------------------------------------------
@pytest.mark.gpu
def test_near_tie_codebook_sends_short_waves_cells_to_the_resolver(dev, oracle_mod):
    """tie-stress codebook on the B = 2 maps that have short waves: every token's two best scores tie, so every cell's owner is
    undecided and queues a record, and the resolver's codes must be the oracle's (the first index of the tied pair).  Where a
    workgroup has more than 64 owners its shard fills and WHICH owners are listed instead is the order the waves draw their slots
    in (tests/test_routed_copies.py), so only the number queued is compared between the forms.  K = 64: staged at B = 2."""
    for case in ("none_fine", "boundary_8", "mixed_row_pairs"):
        i = DUAL_NAMES.index(case)
        f2, f1 = _run_dual(dev, oracle_mod, 64, slice(2 * i, 2 * i + 2), "staged", tie=True)
        assert f2[0] > 0 and f1[0] == f2[0], (case, f2, f1)


@pytest.mark.gpu
def test_full_shards_send_short_waves_coarse_cells_to_the_exact_list(dev, oracle_mod):
    """queue overflow in short waves.  The record capacity is a function of N (64 records per shard, 64 shards, up to 32768 tokens).
    17 all-coarse images, tie-stress codebook, K = 1024: EVERY wave is short (even rows have 16 real columns, odd rows none), every
    even row's 16 owners want a record: 32 per workgroup, 136 workgroups on 64 shards, so eight shards are asked for 96 and each turns
    32 owners away, whichever they are; every one of them lists its 4 positions.  Both counts are functions of the inputs."""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_dual
    K, B = 1024, 17
    assert _form(B, K) == "staged" and max(B * 1024 // 8, 4096) // 64 == 64 and B * 8 == 136
    E = _tie_codebook(K)
    hc = synth.z_tokens(E, B, 16, 16, 4500)
    hf = synth.z_tokens(E, B, 32, 32, 4501)
    ent = np.full((B, 16, 16), np.float32(THR - 1.0), np.float32)
    og = oracle_mod.entropy_gate(ent, THR)
    o_sel = oracle_mod.route_select_dual(og, hc, hf)
    o = oracle_mod.vq_assign_nchw(o_sel["h_dual"], E, o_sel["codebook_mask"])
    t = _t(dev)
    tE, te = t(E), t(ent)
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    with torch.no_grad():
        r2 = vq_assign_routed_dual(t(hc), t(hf), tE, p2, entropy=te, threshold=THR)
        f2 = p2.fallback_count()
        r1 = vq_assign_routed_dual(_off(hc, dev), _off(hf, dev), tE, p1, entropy=te, threshold=THR)
        f1 = p1.fallback_count()
    _check(r2, og, o_sel, o, oracle_mod)
    _check(r1, og, o_sel, o, oracle_mod)
    _same_bits(r2, r1)
    assert f2 == f1 == (8 * 64 + 56 * 64, 8 * 32 * 4), (f2, f1)
