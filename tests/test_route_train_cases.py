"""CPU: the case table of the training-mode routing tail's shape tests (tests/_route_train_ref.py) is what it claims to be.
  * every edge of csrc/router_train.hip that tests/test_route_train_shapes.py is there for is reached by a row, by the restated
    host arithmetic (slab rule, split-K chunk, nq, tile counts); the restated lines are found in the source, so a retuned
    constant sends its author back to the table;
  * the restated workspace layout equals dvq_route_train_workspace_bytes (a host function) on every row;
  * the decisions are clear on the reference alone: after the nudge every perturbed float64 top-2 margin is >= 1e-3, the fp32
    torch chain takes the float64 decisions in every cell, every grain is chosen (but in the 1-cell row): no cell is ever left
    out of a comparison, and this fails instead of skipping."""
import copy
import os
import re

import pytest
import torch

from dynamicvectorquantization_amd import _lib
from tests import _route_train_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = list(range(len(R.CASES)))
IDS = [R.case_id(r) for r in R.CASES]


def test_host_arithmetic_is_the_one_restated():
    src = open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "router_train.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    hint = " -- router_train.hip changed its host arithmetic: restate it in tests/_route_train_ref.py and rebuild CASES for it"
    for line in ("#define RT_NS_MAX %d" % R.RT_NS_MAX,
                 "long s = (N + 511) / 512;",
                 "return (int)(s < 1 ? 1 : (s > RT_NS_MAX ? RT_NS_MAX : s));",
                 "int kc = (K + ns - 1) / ns; kc = (kc + 15) / 16 * 16; const int nz = (K + kc - 1) / kc;",
                 "int kc = (int)((Ncells + ns - 1) / ns); kc = (kc + 15) / 16 * 16; const int nz = (int)((Ncells + kc - 1) / kc);",
                 "dim3 grid((N + 63) / 64, (M + 63) / 64, nz);",
                 "const int nq = Wo <= 256 ? 256 / Wo : 1;",
                 "const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);",
                 "const int c0 = blockIdx.x * 32, k0 = blockIdx.y * 32, b = blockIdx.z;",
                 "for (int k0 = kb; k0 < ke; k0 += 16) {",
                 "const int Gp = a.groups > 0 ? a.groups : a.C / 8;"):
        assert line in flat, line + hint


def test_case_table_reaches_the_edges_it_names():
    geo = [R.geometry(r) for r in R.CASES]
    some = lambda pred: any(pred(g) for g in geo)
    # the 64 x 64 GEMM tile edges
    assert some(lambda g: g["H"] > 0 and g["N"] % 64 != 0 and g["m_tiles"] >= 2), "m < M in a second M tile"
    assert some(lambda g: g["H"] > 64 and g["H"] % 64 != 0), "n < N in a second N tile of the hidden layer"
    assert some(lambda g: g["H"] > 0 and g["F"] > 64 and g["F"] % 64 != 0 and g["n_tiles_F"] >= 4), "n < N, dX = dA W1"
    assert some(lambda g: g["H"] > 0 and g["F"] % 16 != 0), "k < ke: F no multiple of the 16-step"
    assert some(lambda g: g["F"] % 32 != 0)
    assert some(lambda g: g["H"] > 0 and g["H"] % 16 != 0), "k < ke in dX = dA W1"
    # 32 x 32 transposes with partial tiles, in cells and in features
    assert some(lambda g: g["ncell"] % 32 != 0 and g["ncell"] > 32) and some(lambda g: g["ncell"] < 32)
    assert some(lambda g: g["F"] % 32 != 0 and g["F"] > 32) and some(lambda g: g["F"] < 32)
    # one wave per cell, four per workgroup
    assert some(lambda g: g["N"] % 4 != 0 and g["N"] > 4) and some(lambda g: g["N"] == 1)
    # rt_dgg_kernel
    assert some(lambda g: g["Wo"] <= 256 and 256 % g["Wo"] != 0)
    assert some(lambda g: g["nq"] > g["C"])
    assert some(lambda g: g["Wo"] > 256 and g["nb"] == 2) and some(lambda g: g["Wo"] > 256 and g["nb"] == 3)
    assert all(g["nq"] == 1 for g in geo if g["Wo"] > 256)
    # channels per group
    assert some(lambda g: g["groups"] > 0 and g["cpg"] == 1)
    assert some(lambda g: g["groups"] > 0 and g["cpg"] > 1 and g["cpg"] % 2 == 1)
    assert some(lambda g: g["groups"] == 0 and g["C"] // 8 > 1), "pseudo-groups of the pool kernel"
    # B = 1, hidden width, tau, hc != wc, every gate form for both branch counts that have it
    assert some(lambda g: g["B"] == 1) and some(lambda g: g["B"] > 1 and g["B"] % 2 == 1)
    assert some(lambda g: g["H"] > 0 and g["H"] != g["F"] and g["H"] % 64 != 0)
    assert some(lambda g: g["H"] > 0 and g["H"] < g["F"]) and some(lambda g: g["H"] > 0 and g["H"] == g["F"])
    assert some(lambda g: g["tau"] < 1) and some(lambda g: g["tau"] > 1)
    assert all(g["hc"] != g["wc"] for g in geo if g["ncell"] > 16)
    assert {(g["nb"], g["act"]) for g in geo} == {(2, 0), (2, 1), (3, 0), (3, 1), (3, 2)}
    # split-K: more than one slab with a partial last one; the cap
    assert some(lambda g: g["nz"] >= 2 and g["last_slab"] < g["kc"] and g["ns"] < R.RT_NS_MAX)
    assert some(lambda g: (g["N"] + 511) // 512 > R.RT_NS_MAX and g["nz"] == R.RT_NS_MAX and g["last_slab"] < g["kc"])
    assert some(lambda g: g["ns"] == 1)
    # the rows the shape tests name by index
    assert geo[R.ROW_ONE_CELL]["N"] == 1 and geo[R.ROW_105]["N"] == 105 and geo[R.ROW_F24]["F"] == 24
    assert geo[R.ROW_WO258]["Wo"] == 258 and geo[R.ROW_N513]["N"] == 513
    assert geo[R.ROW_N513]["nz"] == 2 and geo[R.ROW_N513]["kc"] == 272
    assert geo[R.ROW_N8320]["N"] == 8320 and geo[R.ROW_N8320]["kc"] == 528 and geo[R.ROW_N8320]["nz"] == 16
    assert R.geometry(R.CASE_NO_UPDATE)["N"] == 105 and R.CASE_NO_UPDATE[0] == 2
    assert len(set(IDS)) == len(IDS)
    # what the ABI accepts (dvq_abi.hip: route_train_args)
    for g in geo:
        assert g["C"] % 8 == 0 and g["F"] <= 1280 and g["H"] <= 1280 and g["Wo"] <= 4096
        assert g["groups"] == 0 or g["C"] % g["groups"] == 0


@pytest.mark.parametrize("row", R.CASES + [R.CASE_NO_UPDATE], ids=IDS + ["no-update"])
def test_workspace_restatement_equals_the_library(row):
    g = R.geometry(row)
    want = R.rt_layout_total(g["nb"], g["B"], g["C"], g["hc"], g["wc"], g["groups"], g["H"])
    got = _lib.lib.dvq_route_train_workspace_bytes(g["nb"], g["B"], g["C"], g["hc"], g["wc"], g["groups"], g["H"])
    assert got == want, "rt_layout changed: restate it in tests/_route_train_ref.py and look at CASES again"


@pytest.mark.parametrize("i", ROWS, ids=IDS)
def test_decisions_stay_clear(i):
    inp, ref = R.case(i)
    g = inp.geo
    z = inp.logits64 + inp.gumbels.double()
    assert float(R.margin(z).min()) >= R.MARGIN
    # a margin below 1e-3 has probability 2e-3 * (the density of the top-2 difference at 0, below 1/2): about N / 1000 cells
    assert inp.nudged <= max(1, g["N"] // 1000), "%d of %d cells nudged" % (inp.nudged, g["N"])
    assert torch.equal(ref["indices"], z.argmax(-1))
    t32 = R.run_torch32(inp, torch.device("cpu"))
    assert torch.equal(t32["indices"], ref["indices"]), "the fp32 chain decides differently from float64"
    assert torch.equal(t32["gate"] == 0, ref["gate"] == 0)
    if g["N"] > 1:
        assert sorted(ref["indices"].unique().tolist()) == list(range(g["nb"])), "pick another seed: a grain is never chosen"
    # the reference is a reference: finite, and the fp32 chain sits at fp32 noise from it (1e-5 of the tensor's maximum)
    for n, r in ref["grads"].items():
        assert bool(torch.isfinite(r).all()) and float(r.abs().max()) > 0, n
        assert float((t32["grads"][n].double() - r).abs().max()) <= 1e-5 * float(r.abs().max()), n


def test_no_update_row_has_clear_logit_margins():
    inp, ref = R.case(-1)
    assert inp.gumbels is None and not inp.update_router
    assert float(R.margin(inp.logits64).min()) >= R.MARGIN, "pick another SEED_NO_UPDATE"
    assert torch.equal(ref["indices"], inp.logits64.argmax(-1))
    assert torch.equal(ref["gate"], inp.logits64.permute(0, 3, 1, 2))
    t32 = R.run_torch32(inp, torch.device("cpu"))
    assert torch.equal(t32["indices"], ref["indices"])
    assert sorted(ref["indices"].unique().tolist()) == [0, 1]


def test_router64_is_the_module_in_float64():
    """the written-out float64 router against the module under test cast to float64 (torch's own GroupNorm / AvgPool / Linear):
    the restatement states the same formula"""
    for i in (R.ROW_105, R.ROW_F24, 3, 4, 9):
        inp, _ = R.case(i)
        hs = [h.detach().double() for h in inp.hs]
        with torch.no_grad():
            want = inp._call(copy.deepcopy(inp.router).double(), hs)
        assert float((want - inp.logits64).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), R.case_id(R.CASES[i])
