"""CPU: the case table of the feature-router gate's shape tests (tests/_gate_ref.py) is what it claims to be.
  * for a device of 256 CUs every row reaches the edge it names, by the restated host arithmetic of csrc/router_gate.hip; the
    restated lines are found in the source, so a retuned constant sends its author back to the table;
  * the restated workspace and prep sizes equal dvq_router_gate_workspace_bytes / dvq_router_gate_prep_bytes (host functions), and
    the restated LDS bytes of the direct form agree with what the ABI accepts on both sides of the limit;
  * the inputs are fit for the argmax condition: the fp32 torch chain on the CPU takes float64's argmax on every cell whose float64
    top-2 margin exceeds the rule's threshold, at most 1 % of a row's cells fall under it, and every grain is chosen somewhere in
    every row of more than 32 cells."""
import os
import re

import pytest
import torch

from dynamicvectorquantization_amd import _lib
from tests import _gate_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def test_host_arithmetic_is_the_one_restated():
    csrc = os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc")
    flat = re.sub(r"\s+", " ", open(os.path.join(csrc, "router_gate.hip")).read())
    hint = " -- router_gate.hip changed its host arithmetic: restate it in tests/_gate_ref.py and look at CASES again"
    for line in ("#define GATE_NW %d" % G.GATE_NW,
                 "const bool steps = nb == 2 ? (S16 == 8 || S16 == 16 || S16 == 24 || S16 == 32) : (S16 == 12 || S16 == 24 || S16 == 48);",
                 "return act != 0 && groups > 0 && cpg % 8 == 0 && cpg <= 64 && (size_t)nb * cpg * hc * wc * 4 <= 48 * 1024 && F % 16 == 0 && steps;",
                 "return ((size_t)32 * Fp + (size_t)(1 + nb) * Hid) * sizeof(float);",
                 "const bool cached = (size_t)B * C * hc * fs * wc * fs * sizeof(float) <= DVQ_CACHED_MAX_BYTES;",
                 "if (a.vec && (Wb & 3) == 0) {",
                 "constexpr int CH = (DVQ_GEMM_CH16 && S % 16 == 0) ? 16 : ((S % 8 == 0) ? 8 : 4);",
                 "constexpr int RING = (CH == 16) ? 4 : 8;",
                 "constexpr bool PIPE = (G == 2) && (S >= 20);",
                 "const int HG = (Hid + 127) / 128; int CG = ncu / HG; if (CG < 1) CG = 1; if (CG > nblocks) CG = nblocks;",
                 "const int nmine = (nblocks - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;",
                 "if ((ncell & 31) != 0)",
                 "for (int h0 = 0; h0 < HG; h0 += 24) {",
                 "const size_t shmem2 = ((size_t)2 * 32 * Fp + (size_t)(1 + nb) * Hid) * sizeof(float);",
                 "const bool cb2 = act != 0 && shmem2 <= DVQ_GATE_LDS_MAX - 256 && ncell >= 64L * ncu;",
                 "if ((S & 3) == 0) {",
                 "return align256r((size_t)((Hid + 127) / 128) * 4 * B * hc * wc * nb * sizeof(float));"):
        assert line in flat, line + hint
    common = re.sub(r"\s+", " ", open(os.path.join(csrc, "dvq_common.h")).read())
    assert "#define DVQ_CACHED_MAX_BYTES ((size_t)64 << 20)" in common and G.CACHED_MAX_BYTES == 64 << 20
    assert "#define DVQ_GATE_LDS_MAX (160 * 1024 - 256)" in re.sub(r"\s+", " ", open(os.path.join(csrc, "launchers.h")).read())
    assert G.GATE_LDS_MAX == 160 * 1024 - 256


def test_case_table_reaches_the_edges_it_names():
    d = {c[0]: G.dispatch(c, 256) for c in G.CASES}
    assert len(set(G.NAMES)) == len(G.NAMES)
    r = d["r01"]       # S = 1; one block of 2 cells; the wave sums [8 waves][1][2 logits][32 cells] exactly fill the 32 x Fp tile
    assert not r["gemm_form"] and r["S"] == 1 and r["ncell"] == 2 and r["grid"] == 1 and not r["cb2"]
    assert G.GATE_NW * 1 * r["nb"] * 32 * 4 == 32 * r["Fp"] * 4
    r = d["r02"]       # padded k, untiled loop
    assert not r["gemm_form"] and (r["F"], r["Fp"], r["S"]) == (24, 32, 2) and not r["pipelined"] and r["act"] == 2
    r = d["r03"]       # padded k; hidden % 32 = 8; mixed pooling
    assert not r["gemm_form"] and (r["F"], r["Fp"]) == (120, 128) and r["Hid"] % 32 == 8 and r["T"] == 3
    assert r["vec"] == [False, True, True] and r["pipelined"]
    r = d["r04"]       # single Linear over padded features
    assert r["act"] == 0 and (r["F"], r["Fp"]) == (216, 224) and r["Hid"] == 32 and not r["gemm_form"] and r["hidden_arg"] == 0
    r = d["r05"]       # one row tile, half masked, three idle waves
    assert r["gemm_form"] and (r["nb"], r["S16"]) == (2, 8) and r["T"] == 1 and r["Hid"] == 16 and r["HG"] == 1 and r["idle_waves"] == 3
    assert not r["PIPE"] and r["CH"] == 8 and r["memset"]
    r = d["r06"]       # two hidden groups, the last with one idle wave and a partial tile
    assert r["gemm_form"] and r["HG"] == 2 and r["T"] == 7 and r["idle_waves"] == 1 and r["Hid"] % 32 == 8 and r["S16"] == 8
    r = d["r07"]       # <2,24>, PIPE, one block exactly
    assert r["gemm_form"] and (r["nb"], r["S16"]) == (2, 24) and r["PIPE"] and r["CH"] == 8 and r["nblocks"] == 1 and not r["memset"]
    r = d["r08"]       # <3,24>, ragged last block
    assert r["gemm_form"] and (r["nb"], r["S16"]) == (3, 24) and not r["PIPE"] and r["memset"] and r["nblocks"] == 1 and r["act"] == 2
    r = d["r09"]       # <2,32> PIPE, 69 blocks over 64 workgroups
    assert r["gemm_form"] and (r["nb"], r["S16"]) == (2, 32) and r["PIPE"] and r["CH"] == 16 and r["RING"] == 4
    assert (r["nblocks"], r["HG"], r["CG"]) == (69, 4, 64) and r["nmine"] == [1, 2] and r["memset"]
    a, b = d["r10a"], d["r10b"]      # either side of the 48 KiB pooling-LDS limit
    assert a["gemm_form"] and a["pool_lds"] == 48 * 1024 and not b["gemm_form"] and b["nb"] * b["cpg"] * b["hc"] * b["wc"] * 4 > 48 * 1024
    assert (a["nb"], a["S16"]) == (2, 8) and a["nblocks"] == 48 and a["nmine"] == [1] and b["pipelined"] and not b["cb2"]
    r = d["r11"]       # direct form, 100 row tiles over 8 waves
    assert not r["gemm_form"] and r["T"] == 100 and r["tiles_per_wave"] == 13 and r["T"] % G.GATE_NW != 0 and r["lds"] <= G.GATE_LDS_MAX
    assert r["shmem"] == 128 * 64 + 4 * 3 * 3200 and r["pipelined"]
    r = d["r12"]       # 100 slices in the finalize kernel
    assert r["gemm_form"] and r["HG"] * 4 == 100 and r["HG"] * 4 > 4 * 24 and r["nblocks"] == 1 and r["CG"] == 1 and r["S16"] == 8
    r = d["r13"]       # cb2, ragged last workgroup, odd row length
    assert not r["gemm_form"] and r["cb2"] and r["ncell"] >= 64 * 256 and r["ncell"] % 64 not in (0, 32) and r["last_cells"] > 32
    assert r["vec"] == [False, False] and r["wc"] % 2 == 1 and r["cached"]
    r = d["r14"]       # the non-temporal pooling pass, GEMM form
    assert r["gemm_form"] and r["pool_kernel"] == (True, True) and (r["nb"], r["S16"]) == (2, 8)
    r = d["r15"]       # ... and direct form, with cb2
    assert not r["gemm_form"] and r["pool_kernel"] == (False, True) and r["cb2"]
    smaller = G.dispatch(("x", 2, 256, 64, 16, 16, "none", G.SILU, None, 0, None, ""), 256)
    assert smaller["cached"], "257 images are the smallest batch of this shape that crosses the 64 MiB rule"
    r = d["r16"]
    assert r["gemm_form"] and r["groups"] == 8 and G.row("r16")[10] == (8.0, 64.0)
    r = d["r17"]       # whole-octet groups, F % 16 == 0, but S16 = 12 exists for three branches only
    assert not r["gemm_form"] and r["cpg"] % 8 == 0 and r["F"] % 16 == 0 and r["F"] // 16 == 12 and r["pipelined"]
    # what the ABI accepts (dvq_abi.hip: dvq_router_gate_f32)
    for r in d.values():
        assert r["C"] % 8 == 0 and r["F"] <= 1280 and r["lds"] <= G.GATE_LDS_MAX
        assert r["groups"] == 0 or (r["C"] % r["groups"] == 0 and (r["cpg"] * r["hc"] * r["wc"]) % 4 == 0)
    assert {(r["pool_kernel"]) for r in d.values()} == {(False, False), (False, True), (True, False), (True, True)}
    for name in G.ABI_ROWS + G.NAN_ROWS:
        assert name in d


@pytest.mark.parametrize("c", G.CASES, ids=G.NAMES)
def test_size_restatement_equals_the_library(c):
    d = G.dispatch(c)
    hint = "the layout changed: restate it in tests/_gate_ref.py and look at CASES again"
    assert _lib.lib.dvq_router_gate_workspace_bytes(*G.abi_size_args(d)) == d["ws_bytes"], hint
    if d["act"] != 0:
        assert _lib.lib.dvq_router_gate_prep_bytes(d["nb"], d["C"], d["Hid"]) == d["prep_bytes"], hint


def test_lds_restatement_agrees_with_the_abi_on_both_sides_of_the_limit():
    """triple routers with the default hidden width: C = 376 is the widest the direct form holds, C = 384 is refused"""
    ws = _lib.lib.dvq_router_gate_workspace_bytes
    for C, fits in ((376, True), (384, False)):
        lds = G.direct_lds_bytes(3, C, 4, 4, 0, 3 * C, 1)
        assert (lds <= G.GATE_LDS_MAX) == fits, (C, lds)
        got = ws(3, 2, C, 4, 4, 0, 3 * C)
        assert (got != 0) == fits and (not fits or got == G.ws_bytes(3, 2, C, 4, 4, 3 * C)), (C, got)
    assert G.direct_lds_bytes(3, 384, 4, 4, 0, 1152, 1) == 165888 and G.direct_lds_bytes(2, 640, 4, 4, 0, 32, 0) == 164224
    assert ws(2, 2, 640, 4, 4, 0, 0) == 0 and ws(2, 2, 632, 4, 4, 0, 0) != 0          # single-layer, dual
    assert ws(2, 2, 8, 4, 4, 0, 16384) == 0 and ws(2, 2, 8, 4, 4, 0, 8192) != 0        # a small router, a very wide hidden layer
    # the GEMM form's LDS does not grow with the hidden layer: the same width is served behind whole-octet GroupNorm groups
    assert G.direct_lds_bytes(2, 64, 4, 4, 8, 16384, 1) == 0 and ws(2, 2, 64, 4, 4, 8, 16384) != 0


@pytest.mark.parametrize("name", G.NAMES)
def test_inputs_are_fit_for_the_argmax_condition(name):
    inp = G.case(name)
    ref, geo = inp.logits64, inp.geo
    assert tuple(ref.shape) == (geo["B"], geo["hc"], geo["wc"], geo["nb"]) and bool(torch.isfinite(ref).all())
    t32 = G.run_torch32(inp, CPU)
    ek, et, fl = G.image_errors(t32, t32, ref)
    clear = G.clear_cells(ref, et, fl)
    assert torch.equal(t32.argmax(-1)[clear], ref.argmax(-1)[clear]), "the fp32 chain decides differently from float64 on a clear cell"
    unclear = int((~clear).sum())
    print("%s: %d of %d cells under the threshold, err_torch32 %.3g, max |ref| %.3g" % (name, unclear, geo["ncell"], float(et.max()),
                                                                                       float(ref.abs().max())))
    assert unclear * 100 <= geo["ncell"], "pick another seed: %d of %d cells under the margin threshold" % (unclear, geo["ncell"])
    if geo["ncell"] > 32:
        assert sorted(ref.argmax(-1).unique().tolist()) == list(range(geo["nb"])), "pick another seed: a grain is never chosen"
    # the reference is a reference: the fp32 chain sits at fp32 noise from it (the offset row: at the noise of its large means)
    assert float(et.max()) <= (1e-5 if name != G.ROW_OFFSET else 1e-3) * max(1.0, float(ref.abs().max()))


def test_router64_is_the_module_in_float64():
    import copy
    for name in ("r02", "r03", "r04", "r06", "r16"):
        inp = G.case(name)
        with torch.no_grad():
            want = inp.call(copy.deepcopy(inp.router).double(), [h.double() for h in inp.hs])
        assert float((want - inp.logits64).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max())), name
