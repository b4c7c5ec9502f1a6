"""CPU: fp16 / bf16 branch features at the C ABI and in the gate's case table (include/dvq.h 0.19.0).

(1) DVQ_FEATURES(dtype), OR-ed into `gate_dtype` of dvq_route_select_dual_f32 / dvq_route_select_triple_f32 and into `activation`
    of dvq_router_gate_f32, reaches validation: a flagged call with B = 0 answers "sizes must be positive" (before 0.19.0 the enum
    check answered `gate_dtype 256` / `unknown activation 257`); an unknown enumerator under the flag keeps the words pinned in
    tests/golden/abi_rejections.json for its low byte; dtype bits 3 and misaligned 16-bit pointers are DVQ_EINVAL in words of
    their own; the entry points that stay float32-only (the training tail, the conv-fused select, the routed assigns in all
    forms) refuse the flag by their own enumerator checks.  The calls run in a child process that sees no GPU, on fake pointers,
    through the replay of tools/gen_golden_abi_rejections.py: a check that is lost shows as a wrong status, never as a kernel.
(2) Every row of tests/_gate_ref.CASES stays fit for the argmax rule when its branches are rounded to fp16 / bf16: at most 1 % of
    the cells under the margin, every grain chosen, the fp32 torch chain agreeing with float64 on every clear cell -- the three
    conditions of tests/test_router_gate_cases.py::test_inputs_are_fit_for_the_argmax_condition, on the rounded values."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest
import torch

from tests import _gate_ref as G
from tests import _route_x16_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tools", "gen_golden_abi_rejections.py")
CPU = torch.device("cpu")
EINVAL = -1
F16, BF16, BITS3 = 1 << 8, 2 << 8, 3 << 8                     # DVQ_FEATURES(DVQ_DTYPE_F16 / DVQ_DTYPE_BF16), dtype bits 3


def _tool():
    spec = importlib.util.spec_from_file_location("gen_golden_abi_rejections", TOOL)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _replay(tmp_path, calls):
    """[(rc, message)] of the (fn, {parameter: value}) calls; what is not named: pointers 256, numbers 1, stream 0 (the tool's rule)"""
    tool = _tool()
    tool.ROWS[:] = calls
    table = tool.rows(tool.prototypes())
    path = os.path.join(str(tmp_path), "calls.json")
    json.dump(table, open(path, "w"))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, TOOL, "--replay", path], env=env, check=True, capture_output=True, text=True, timeout=120).stdout
    got = [tuple(r) for r in json.loads(out)]
    assert len(got) == len(calls)
    return got


def test_lib_restates_the_flag():
    from dynamicvectorquantization_amd import _lib
    header = open(os.path.join(ROOT, "include", "dvq.h")).read()
    assert "#define DVQ_FEATURES(dtype) ((dtype) << 8)" in header and " 0.19.0 " in header
    assert _lib.lib.dvq_version() >= 1900
    assert (_lib.FEATURES(torch.float16), _lib.FEATURES(torch.bfloat16), _lib.FEATURES(torch.float32)) == (F16, BF16, 0)


def test_flags_reach_validation(tmp_path):
    d = dict
    gate2 = d(num_branches=2, h_median=0)
    calls, want = [], []

    def add(fn, named, rc, message):
        calls.append((fn, named))
        want.append((rc, message if message is None else fn + ": " + message))

    for flag in (F16, BF16):
        for sel in ("dvq_route_select_dual_f32", "dvq_route_select_triple_f32"):
            for kind in (0, 1):                                # DVQ_GATE_F32, DVQ_GATE_I64
                add(sel, d(gate_dtype=kind | flag, B=0), EINVAL, "sizes must be positive")
            add(sel, d(gate_dtype=5 | flag), EINVAL, "gate_dtype 5")
            add(sel, d(gate_dtype=flag, h_fine=257), EINVAL, "16-bit features must be 2-byte aligned")
            add(sel, d(gate_dtype=flag, h_out=257), EINVAL, "16-bit features must be 2-byte aligned")
        add("dvq_route_select_triple_f32", d(gate_dtype=flag, h_median=257), EINVAL, "16-bit features must be 2-byte aligned")
        for act in (0, 1, 2):
            add("dvq_router_gate_f32", d(gate2, activation=act | flag, B=0), EINVAL, "sizes must be positive")
        add("dvq_router_gate_f32", d(gate2, activation=9 | flag), EINVAL, "unknown activation 9")
        add("dvq_router_gate_f32", d(gate2, activation=1 | flag, h_fine=260), EINVAL, "16-bit features must be 8-byte aligned")
        # what stays float32-only refuses the flag with its own enumerator check
        add("dvq_route_train_forward_f32", d(gate2, activation=1 | flag), EINVAL, "unknown activation %d" % (1 | flag))
        add("dvq_route_train_backward_f32", d(gate2, activation=1 | flag), EINVAL, "unknown activation %d" % (1 | flag))
        add("dvq_qconv_select_f32", d(gate2, gate_kind=flag), EINVAL, "gate_kind %d" % flag)
        for routed in ("dvq_vq_assign_routed_dual_f32", "dvq_vq_assign_routed_triple_f32", "dvq_vq_assign_routed_qconv_dual_f32",
                       "dvq_vq_assign_routed_qconv_triple_f32", "dvq_vq_assign_routed_fold_dual_f32", "dvq_vq_assign_routed_fold_triple_f32"):
            add(routed, d(gate_kind=1 | flag), EINVAL, "gate_kind %d" % (1 | flag))
    message3 = "DVQ_FEATURES dtype 3 (0 = float32, DVQ_DTYPE_F16 = 1, DVQ_DTYPE_BF16 = 2)"
    add("dvq_route_select_dual_f32", d(gate_dtype=BITS3), EINVAL, message3)
    add("dvq_route_select_triple_f32", d(gate_dtype=1 | BITS3), EINVAL, message3)
    add("dvq_router_gate_f32", d(gate2, activation=1 | BITS3), EINVAL, message3)
    # a negative value carries no flag: an unknown enumerator, as a whole
    add("dvq_route_select_dual_f32", d(gate_dtype=-1), EINVAL, "gate_dtype -1")
    add("dvq_router_gate_f32", d(gate2, activation=-256), EINVAL, "unknown activation -256")
    got = _replay(tmp_path, calls)
    for (fn, named), g, w in zip(calls, got, want):
        assert g == w, (fn, named, g, w)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("name", G.NAMES)
def test_rounded_rows_stay_fit_for_the_argmax_condition(name, dtype):
    inp = X.rounded(name, dtype)
    ref, geo = inp.logits64, inp.geo
    for h in inp.hs:
        assert bool(torch.isfinite(h).all()) and torch.equal(h.to(dtype).float(), h)
    assert tuple(ref.shape) == (geo["B"], geo["hc"], geo["wc"], geo["nb"]) and bool(torch.isfinite(ref).all())
    t32 = G.run_torch32(inp, CPU)
    ek, et, fl = G.image_errors(t32, t32, ref)
    clear = G.clear_cells(ref, et, fl)
    assert torch.equal(t32.argmax(-1)[clear], ref.argmax(-1)[clear]), "the fp32 chain decides differently from float64 on a clear cell"
    unclear = int((~clear).sum())
    print("%s %s: %d of %d cells under the threshold, err_torch32 %.3g, max |ref| %.3g" % (name, dtype, unclear, geo["ncell"],
                                                                                         float(et.max()), float(ref.abs().max())))
    assert unclear * 100 <= geo["ncell"], "%d of %d cells under the margin threshold" % (unclear, geo["ncell"])
    if geo["ncell"] > 32:
        assert sorted(ref.argmax(-1).unique().tolist()) == list(range(geo["nb"])), "a grain is never chosen"
