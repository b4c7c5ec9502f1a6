"""The copies of a coarse cell in the LDS-staged routed pass 1 (csrc/dvq_pass1.h, SEL == 2): every output position of a coarser
cell but its first feeds ZERO operands to the code loop and takes (best, second, code) from the lane that owns the cell, behind
the loop.  Nothing the op returns may change, so every GPU check here is bit-exact against the CPU oracle's select + assign
(loss 1e-5) and, differentially, against the per-lane form (SEL == 1), which scores every position's own vector: the op takes
that form when a branch tensor is not 16-byte aligned, so the same tensors are handed over once more as views at a 4-byte
storage offset.

Which form a shape takes is restated here from `pass1_plan` / `split_slices` (csrc/vq_assign_filter.hip) and asserted per case:
32-wide output grids take the staged form from 65 token blocks on; (4, 2, 16) and (5, 3, 8) are 32 wide but have 4 / 15 blocks,
so the small-batch split form (per-lane select) serves them -- they are run all the same, and (66, 2, 16) / (22, 3, 8) put the
same 4- and 12-row images through the staged form."""
import numpy as np
import pytest
import torch

from tests import _cases as C

K, D = 300, 256


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


def _form(B, rows, K, aligned=True):
    """pass1_plan for a routed op without conv on a 32-wide output grid of `rows` rows per image"""
    nb = (B * rows * 32 + 127) // 128
    tiles = (K + 31) // 32
    ks = 1
    if nb <= 64:                                                  # DVQ_SPLIT_MAX_BLOCKS
        ks = 8                                                    # DVQ_SPLIT_MAX_SLICES
        while ks > 1 and (nb * ks > 256 or tiles // ks < 2):
            ks >>= 1
    if ks > 1:
        return "split"
    return "staged" if aligned and (rows * 32) % 128 == 0 else "per-lane"


def _codebook(K, D, seed=91):
    from dynamicvectorquantization_amd import synth
    E = synth.codebook_trained(K, D, seed=seed)
    E[7] = E[3]                                                   # duplicate code: the first index wins
    return E


def _grains(G, B, hc, wc, seed):
    """grain per cell [B, hc, wc] (0 = coarsest ... G - 1 = fine), one pattern per image, iid from image 8 on"""
    from dynamicvectorquantization_amd import synth
    F = G - 1
    yy, xx = np.meshgrid(np.arange(hc), np.arange(wc), indexing="ij")
    pats = [np.zeros((hc, wc), np.int64),                         # all coarse (triple: every 4 x 4 cell is 15 copies)
            np.full((hc, wc), F, np.int64),                       # all fine
            np.where((yy + xx) % 2 == 0, 0, F),                   # checkerboard of cells
            np.zeros((hc, wc), np.int64),                         # one fine cell in a coarse image
            np.full((hc, wc), F, np.int64),                       # one coarse cell in a fine image
            np.where(yy % 2 == 0, 0, F),                          # alternate cell rows
            (xx + yy) % G,                                        # a cell of every grain inside one workgroup
            np.full((hc, wc), G - 2, np.int64)]                   # all of the 2x-coarser branch (dual: = all coarse)
    pats[3][hc // 2, wc // 3] = F
    pats[4][hc // 2, wc // 3] = 0
    g = np.empty((B, hc, wc), np.int64)
    iid = synth.randint(seed, (B, hc, wc), 2).astype(np.int64) * F if G == 2 else synth.randint(seed, (B, hc, wc), 3).astype(np.int64)
    for b in range(B):
        g[b] = pats[b] if b < len(pats) else iid[b]
    return g


def _gate(g, G):
    return np.stack([g == k for k in range(G)], -1).astype(np.int64)


def _branches(E, G, B, hc, wc, seed):
    """[coarsest, ..., fine] branch tensors"""
    from dynamicvectorquantization_amd import synth
    return [synth.z_tokens(E, B, hc << k, wc << k, seed + k) for k in range(G)]


def _run(G, br, E, prep, gate, **kw):
    from dynamicvectorquantization_amd.quantize import vq_assign_routed_dual, vq_assign_routed_triple
    if G == 2:
        return vq_assign_routed_dual(br[0], br[1], E, prep, gate=gate, **kw)
    return vq_assign_routed_triple(br[0], br[1], br[2], E, prep, gate, **kw)


def _oracle(oracle_mod, G, gate, br, E):
    if G == 2:
        o_sel = oracle_mod.route_select_dual(gate, br[0], br[1])
        h = o_sel["h_dual"]
    else:
        o_sel = oracle_mod.route_select_triple(gate, br[0], br[1], br[2])
        h = o_sel["h_triple"]
    return o_sel, oracle_mod.vq_assign_nchw(h, E, o_sel["codebook_mask"])


def _check(r, o_sel, o, B, oracle_mod):
    assert np.array_equal(r["indices"].cpu().numpy(), o_sel["indices"]), "grain indices"
    assert np.array_equal(r["codebook_mask"].cpu().numpy(), o_sel["codebook_mask"]), "codebook_mask"
    assert np.array_equal(r["codes"].cpu().numpy().reshape(B, -1), o["codes"]), "codes"
    if r["zq"] is not None:
        assert np.array_equal(r["zq"].cpu().numpy(), o["zq"], equal_nan=True), "z_q"
    if r["loss"] is not None:
        assert C.loss_close(float(r["loss"][1]), oracle_mod.vq_loss(o["sqerr"], o["numel"], 0.25)), "loss"


def _same_bits(a, b):
    for k in ("codes", "zq", "indices", "codebook_mask"):
        assert (a[k] is None) == (b[k] is None), k
        if a[k] is not None:
            assert np.array_equal(a[k].cpu().numpy().view(np.int32 if a[k].dtype == torch.float32 else np.int64),
                                  b[k].cpu().numpy().view(np.int32 if b[k].dtype == torch.float32 else np.int64)), k
    assert (a["loss"] is None) == (b["loss"] is None)
    if a["loss"] is not None:
        assert np.array_equal(a["loss"].cpu().numpy().view(np.int32), b["loss"].cpu().numpy().view(np.int32)), "loss bits"


def _both_forms(dev, oracle_mod, G, gate, br, E, B, rows, Kc, listed_is_ordered=False, **kw):
    """the op on aligned tensors (staged form where the plan says so) and on the offset views (per-lane select): each against
    the oracle, and against each other bit for bit, fallback counts included.  -> (staged result, its fallback count)
    listed_is_ordered: the queue overflows and the cells of a shard differ in size -- which owners find the shard full is the
    order in which a workgroup's waves (and two workgroups on one shard) draw their slots, so the number of LISTED positions
    is not a function of the inputs in either form; the number of queued records is, and is compared."""
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    t = _t(dev)
    o_sel, o = _oracle(oracle_mod, G, gate, br, E)
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    tE = t(E)
    r2 = _run(G, [t(a) for a in br], tE, p2, t(gate), **kw)
    f2 = p2.fallback_count()
    r1 = _run(G, [_off(a, dev) for a in br], tE, p1, t(gate), **kw)
    f1 = p1.fallback_count()
    assert _form(B, rows, Kc, aligned=False) in ("per-lane", "split")
    _check(r2, o_sel, o, B, oracle_mod)
    _check(r1, o_sel, o, B, oracle_mod)
    _same_bits(r2, r1)
    print("fallback_count staged %s per-lane %s" % (f2, f1))
    if listed_is_ordered:
        assert f2[0] == f1[0] and f2[1] > 0 and f1[1] > 0, (f2, f1)
    else:
        assert f2 == f1, (f2, f1)
    return r2, f2


CASES = [(2, (9, 16, 16), 256, "staged"), (2, (4, 2, 16), 256, "split"), (2, (66, 2, 16), 256, "staged"),
         (2, (9, 16, 16), 64, "staged"),
         (3, (10, 8, 8), 256, "staged"), (3, (5, 3, 8), 256, "split"), (3, (22, 3, 8), 256, "staged")]


@pytest.mark.gpu
@pytest.mark.parametrize("G,shape,Dd,form", CASES)
def test_gate_patterns_bit_exact_in_both_forms(dev, oracle_mod, G, shape, Dd, form):
    """explicit int64 gates -- all coarse, all fine, a checkerboard of cells, one fine cell in a coarse image and the reverse,
    alternate cell rows, every grain inside one workgroup, iid -- one pattern per image (ragged batches repeat / cut the list)"""
    B, hc, wc = shape
    rows = hc << (G - 1)
    assert _form(B, rows, K) == form
    E = _codebook(K, Dd)
    br = _branches(E, G, B, hc, wc, 100 * G + hc)
    gate = _gate(_grains(G, B, hc, wc, 7 + hc), G)
    _, (queued, listed) = _both_forms(dev, oracle_mod, G, gate, br, E, B, rows, K)
    assert queued > 0                                             # the resolver had records (owners only)


@pytest.mark.gpu
@pytest.mark.parametrize("G,shape", [(2, (9, 16, 16)), (3, (10, 8, 8))])
def test_special_values_in_the_owner_and_under_it(dev, oracle_mod, G, shape):
    """NaN / +Inf / -Inf / x 1e6 / all-zero in a COARSER-branch vector whose cell is selected: its rep^2 positions take the route
    they always took (exact list for the unscorable ones); the same values in the finer branches UNDER a coarse cell are not
    selected and change nothing"""
    B, hc, wc = shape
    rows = hc << (G - 1)
    assert _form(B, rows, K) == "staged"
    E = _codebook(K, D)
    br = _branches(E, G, B, hc, wc, 300 * G)
    g = _grains(G, B, hc, wc, 31)[::-1].copy()                   # iid images first: the forced cells sit in mixed surroundings
    cy, cx = 2, 3                                                 # a coarse cell, forced to the coarsest branch everywhere
    g[:, cy, cx] = 0

    def poison(a, y, x):
        a[0, 5, y, x] = np.nan
        a[1, :, y, x] = np.inf
        a[2, 9, y, x] = -np.inf
        a[3, :, y, x] *= np.float32(1e6)
        a[4, :, y, x] = 0.0

    poison(br[0], cy, cx)                                         # the owner's vector, images 0 .. 4
    for k in range(1, G):                                         # finer branches under that cell: never selected
        s = 1 << k
        for a_y in range(s):
            poison(br[k][4:], cy * s + a_y, cx * s + (a_y % s))   # images 4 .. 8
    if G == 3:                                                    # ... and a selected MEDIAN vector (rep 2) next to a coarse one
        g[:, 5, 5] = 1
        g[:, 5, 4] = 0
        poison(br[1], 10, 10)
        poison(br[2], 20, 21)                                     # fine values under it: not selected
    gate = _gate(g, G)
    _, (queued, listed) = _both_forms(dev, oracle_mod, G, gate, br, E, B, rows, K)
    assert listed > 0                                             # the exact list was used


@pytest.mark.gpu
@pytest.mark.parametrize("G,shape", [(2, (9, 16, 16)), (3, (10, 8, 8))])
def test_tie_stress_codebook_overflows_whole_cells_to_the_exact_list(dev, oracle_mod, G, shape):
    """a default-initialised codebook whose second half repeats the first (with the usual latents the plain one leaves few
    tokens undecided: 383 of 9216) ties every token exactly, so every cell's owner wants a record and the shards (64 records
    each at these sizes) fill up: whole cells -- all rep^2 positions, listed by the owner -- go to the exact list.
    (1) 17 images of 2x-coarser cells only (dual: all coarse; triple: all median): 32 owners per workgroup, 136 workgroups on
        64 shards, so eight shards are asked for 96 records; every owner turned away lists 4 positions, whichever it is, and
        both counts are functions of the inputs: equal to the per-lane form's.
    (2) the mixed patterns, cells of every size side by side in a shard: WHICH owners are turned away is the order in which the
        waves draw their slots, in either form, so only the number queued is compared (listed: both > 0).
    Bit-exact against the oracle and between the forms in both."""
    from dynamicvectorquantization_amd import synth
    B, hc, wc = shape
    rows = hc << (G - 1)
    Kc, B1 = 1024, 17
    assert _form(B, rows, Kc) == "staged" and _form(B1, rows, Kc) == "staged"
    E = synth.codebook_default_init(Kc, D)
    E[Kc // 2:] = E[:Kc // 2]
    br = _branches(E, G, B1, hc, wc, 500 * G)
    N1 = B1 * rows * 32
    assert max(N1 // 8, 4096) // 64 == 64 and N1 // 128 == 136
    g = np.full((B1, hc, wc), G - 2, np.int64)
    _, (queued, listed) = _both_forms(dev, oracle_mod, G, _gate(g, G), br, E, B1, rows, Kc)
    assert (queued, listed) == (8 * 64 + 56 * 64, 8 * 32 * 4), (queued, listed)
    gate = _gate(_grains(G, B, hc, wc, 53), G)
    _, (queued, listed) = _both_forms(dev, oracle_mod, G, gate, [a[:B] for a in br], E, B, rows, Kc, listed_is_ordered=True)
    assert queued > 0 and listed > 0, (queued, listed)


@pytest.mark.gpu
@pytest.mark.parametrize("G,shape", [(2, (9, 16, 16)), (3, (10, 8, 8))])
def test_codes_only_loss_only_and_fold(dev, oracle_mod, G, shape):
    """the calls without z_q / without the loss, and the folded-conv op (the SEL == 2, FOLD instantiation): staged and per-lane
    forms agree bit for bit; the folded op's codes equal the fused-conv op's"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep
    B, hc, wc = shape
    rows = hc << (G - 1)
    assert _form(B, rows, K) == "staged"
    E = _codebook(K, D)
    br = _branches(E, G, B, hc, wc, 700 * G)
    gate = _gate(_grains(G, B, hc, wc, 71), G)
    r, _ = _both_forms(dev, oracle_mod, G, gate, br, E, B, rows, K, want_zq=False, want_loss=False)
    assert r["zq"] is None and r["loss"] is None
    r, _ = _both_forms(dev, oracle_mod, G, gate, br, E, B, rows, K, want_zq=False)
    assert r["zq"] is None and r["loss"] is not None
    t = _t(dev)
    conv = torch.nn.Conv2d(D, D, 1)
    with torch.no_grad():
        q = np.linalg.qr(synth.normal(711, (D, D)).astype(np.float64))[0].astype(np.float32)
        conv.weight.copy_(torch.from_numpy(np.ascontiguousarray(q).reshape(D, D, 1, 1)))
        conv.bias.copy_(torch.from_numpy(synth.normal(712, (D,), 0.0, 0.1)))
    conv = conv.to(dev).eval()
    tE, tg = t(E), t(gate)
    p2, p1 = _CodebookPrep(), _CodebookPrep()
    f2 = _run(G, [t(a) for a in br], tE, p2, tg, want_loss=False, conv=conv, fold=True)
    c2 = p2.fallback_count()
    f1 = _run(G, [_off(a, dev) for a in br], tE, p1, tg, want_loss=False, conv=conv, fold=True)
    c1 = p1.fallback_count()
    _same_bits(f2, f1)
    assert c2 == c1, (c2, c1)
    r0 = _run(G, [t(a) for a in br], tE, _CodebookPrep(), tg, conv=conv)
    assert torch.equal(f2["codes"], r0["codes"]) and torch.equal(f2["indices"], r0["indices"])
    o_sel, _ = _oracle(oracle_mod, G, gate, br, E)
    assert np.array_equal(f2["indices"].cpu().numpy(), o_sel["indices"])
    assert np.array_equal(f2["codebook_mask"].cpu().numpy(), o_sel["codebook_mask"])


@pytest.mark.parametrize("G,grain,rep", [(2, 1, 1), (2, 0, 2), (3, 2, 1), (3, 1, 2), (3, 0, 4)])
def test_owner_formula_names_the_first_position_of_the_cell(oracle_mod, G, grain, rep):
    """CPU: the hand-over's owner -- wave - (wave % rep), column - (column % rep), for every (row, column) of a workgroup's
    4 x 32 block -- is the first position, in the order pass 1 walks them, that holds the cell's vector in the oracle's select"""
    hc, wc = (2, 16) if G == 2 else (1, 8)                        # one workgroup: 4 output rows of 32 positions
    S = 1 << (G - 1)
    br = [np.arange((hc << k) * (wc << k), dtype=np.float32).reshape(1, 1, hc << k, wc << k) + np.float32(1000 * k) for k in range(G)]
    gate = _gate(np.full((1, hc, wc), grain, np.int64), G)
    sel = oracle_mod.route_select_dual(gate, br[0], br[1]) if G == 2 else oracle_mod.route_select_triple(gate, br[0], br[1], br[2])
    h = sel["h_dual" if G == 2 else "h_triple"][0, 0]
    assert h.shape == (4, 32) and S * hc == 4
    assert np.all(sel["codebook_mask"] == np.float32(1.0 / (rep * rep)))
    flat = h.reshape(-1)
    first = np.array([int(np.nonzero(flat == v)[0][0]) for v in flat]).reshape(4, 32)
    y, x = np.meshgrid(np.arange(4), np.arange(32), indexing="ij")
    owner = (y - (y % rep)) * 32 + (x - (x % rep))
    assert np.array_equal(owner, first)
    assert np.array_equal(owner == y * 32 + x, (y % rep == 0) & (x % rep == 0))   # the lanes whose sel_mask stays positive
