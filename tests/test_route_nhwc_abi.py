"""CPU: channels_last branch features at the C ABI and in the gate's case table (include/dvq.h 0.20.0).

(1) DVQ_NHWC, OR-ed into `gate_dtype` of dvq_route_select_dual_f32 / dvq_route_select_triple_f32 and into `activation` of
    dvq_router_gate_f32, alone and with each DVQ_FEATURES(dtype), reaches validation: a flagged call with B = 0 answers "sizes must
    be positive" (before 0.20.0 bit 12 was read as `DVQ_FEATURES dtype 16`); an unknown enumerator under the flag keeps the words
    pinned in tests/golden/abi_rejections.json for its low byte; a bit above 12 is DVQ_EINVAL in words of its own; dtype bits 3
    answer the pinned `dtype 3` message with and without the layout bit; the entry points that stay NCHW-only (the training tail,
    the conv-fused select, a routed assign) refuse the flag by their own enumerator checks.  The calls run in a child process
    that sees no GPU, on fake pointers, through the replay of tools/gen_golden_abi_rejections.py: a check that is lost shows as a
    wrong status, never as a kernel.
(2) Every row of tests/_gate_ref.CASES that tests/test_route_nhwc.py runs leaves at most 1 % of its cells out of the argmax
    comparison (`_gate_ref.clear_cells` on the float64 reference), for the float32 values and for their fp16 / bf16 roundings: a
    condition on the inputs, so that the GPU test cannot hide a failure behind unclear cells."""
import importlib.util
import json
import os
import re
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
NHWC = 0x1000
F16, BF16, BITS3 = 1 << 8, 2 << 8, 3 << 8
GATE_ROWS = ["r%02d" % i for i in range(1, 10)] + ["r10a", "r10b", "r11", "r12", "r13", "r17"]       # r01 - r13 and r17
GATE_ROWS_F32_ONLY = ["r14", "r15"]                                                                  # > 64 MiB: once, float32


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
    m = re.search(r"^#define DVQ_NHWC \(1 << (\d+)\)", header, flags=re.M)
    assert m and 1 << int(m.group(1)) == NHWC and " 0.20.0 " in header
    assert _lib.lib.dvq_version() == 2000
    assert _lib.NHWC == NHWC
    assert _lib.NHWC & (_lib.FEATURES(torch.float16) | _lib.FEATURES(torch.bfloat16) | 0xFF) == 0


def test_the_layout_flag_reaches_validation(tmp_path):
    d = dict
    gate2 = d(num_branches=2, h_median=0)
    calls, want = [], []

    def add(fn, named, rc, message):
        calls.append((fn, named))
        want.append((rc, message if message is None else fn + ": " + message))

    for flag in (NHWC, NHWC | F16, NHWC | BF16):
        for sel in ("dvq_route_select_dual_f32", "dvq_route_select_triple_f32"):
            for kind in (0, 1):                                # DVQ_GATE_F32, DVQ_GATE_I64
                add(sel, d(gate_dtype=kind | flag, B=0), EINVAL, "sizes must be positive")
            add(sel, d(gate_dtype=5 | flag), EINVAL, "gate_dtype 5")
        for act in (0, 1, 2):
            add("dvq_router_gate_f32", d(gate2, activation=act | flag, B=0), EINVAL, "sizes must be positive")
        add("dvq_router_gate_f32", d(gate2, activation=9 | flag), EINVAL, "unknown activation 9")
        # what stays NCHW-only refuses the flag with its own enumerator check
        add("dvq_route_train_forward_f32", d(gate2, activation=1 | flag), EINVAL, "unknown activation %d" % (1 | flag))
        add("dvq_qconv_select_f32", d(gate2, gate_kind=flag), EINVAL, "gate_kind %d" % flag)
        add("dvq_vq_assign_routed_dual_f32", d(gate_kind=1 | flag), EINVAL, "gate_kind %d" % (1 | flag))
    # 16-bit channels_last features are aligned to their element, as the NCHW ones
    add("dvq_route_select_dual_f32", d(gate_dtype=NHWC | BF16, h_fine=257), EINVAL, "16-bit features must be 2-byte aligned")
    add("dvq_router_gate_f32", d(gate2, activation=1 | NHWC | BF16, h_fine=257), EINVAL,
        "DVQ_NHWC features must be aligned to their element size (2 bytes)")
    add("dvq_router_gate_f32", d(gate2, activation=1 | NHWC, h_coarse=258), EINVAL,
        "DVQ_NHWC features must be aligned to their element size (4 bytes)")
    # bits above the layout bit: words of their own, with and without the flags below them
    for high in (0x2000, 0x4000 | NHWC, 0x10000 | BF16, 0x40000000):
        words = "flag bits 0x%x above DVQ_NHWC (the argument carries an enumerator, DVQ_FEATURES(dtype) and DVQ_NHWC)" % (high & ~0x1FFF)
        add("dvq_route_select_dual_f32", d(gate_dtype=high), EINVAL, words)
        add("dvq_route_select_triple_f32", d(gate_dtype=1 | high), EINVAL, words)
        add("dvq_router_gate_f32", d(gate2, activation=1 | high), EINVAL, words)
    add("dvq_route_select_dual_f32", d(gate_dtype=5 | 0x2000), EINVAL, "gate_dtype 5")       # the enumerator is checked first
    message3 = "DVQ_FEATURES dtype 3 (0 = float32, DVQ_DTYPE_F16 = 1, DVQ_DTYPE_BF16 = 2)"
    for bits in (BITS3, BITS3 | NHWC):
        add("dvq_route_select_dual_f32", d(gate_dtype=bits), EINVAL, message3)
        add("dvq_route_select_triple_f32", d(gate_dtype=1 | bits), EINVAL, message3)
        add("dvq_router_gate_f32", d(gate2, activation=1 | bits), EINVAL, message3)
    # a negative value carries no flag: an unknown enumerator, as a whole
    add("dvq_route_select_dual_f32", d(gate_dtype=-NHWC), EINVAL, "gate_dtype %d" % -NHWC)
    add("dvq_router_gate_f32", d(gate2, activation=-NHWC), EINVAL, "unknown activation %d" % -NHWC)
    got = _replay(tmp_path, calls)
    for (fn, named), g, w in zip(calls, got, want):
        assert g == w, (fn, named, g, w)


ROWS_AND_TYPES = ([(n, torch.float32) for n in GATE_ROWS + GATE_ROWS_F32_ONLY] + [(n, t) for n in GATE_ROWS for t in X.DTYPES])


@pytest.mark.parametrize("name,dtype", ROWS_AND_TYPES, ids=["%s-%s" % (n, str(t).split(".")[-1]) for n, t in ROWS_AND_TYPES])
def test_the_rows_leave_few_cells_unclear(name, dtype):
    inp = G.case(name) if dtype == torch.float32 else X.rounded(name, dtype)
    ref, geo = inp.logits64, inp.geo
    assert tuple(ref.shape) == (geo["B"], geo["hc"], geo["wc"], geo["nb"]) and bool(torch.isfinite(ref).all())
    t32 = G.run_torch32(inp, CPU)
    ek, et, fl = G.image_errors(t32, t32, ref)
    unclear = int((~G.clear_cells(ref, et, fl)).sum())
    print("%s %s: %d of %d cells under the threshold" % (name, dtype, unclear, geo["ncell"]))
    assert unclear * 100 <= geo["ncell"], "%d of %d cells under the margin threshold" % (unclear, geo["ncell"])
