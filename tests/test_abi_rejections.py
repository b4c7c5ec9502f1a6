"""What the C ABI refuses stays refused, with the same status and the same words: tests/golden/abi_rejections.json holds, for every
int-returning entry point of include/dvq.h, calls that argument validation turns down -- per distinct check of the dense assign,
its backward, the EMA statistics and the other assigns, in ladders that also pin WHICH check answers when several arguments are
wrong (tools/gen_golden_abi_rejections.py, which recorded the table, explains them).  dvq.h promises status codes, and callers
match on the message of dvq_last_error_string(), so a refactor of csrc/dvq_abi.hip has to leave both as they were.

The calls run in a child process that sees no GPU: their pointers are fake, and a check that a later edit loses must show as a
wrong rc (the launch fails for want of a device), never as a kernel on those pointers.  No GPU needed."""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE = os.path.join(ROOT, "tests", "golden", "abi_rejections.json")
TOOL = os.path.join(ROOT, "tools", "gen_golden_abi_rejections.py")
# one row per distinct check at the least: assign (f32, x16, flat), backward and EMA pairs, qconv, fold, a dual and a triple routed
# entry, soft, score, both apply_codes, both gumbel, both narrow entries, the two prepares, the router gate
_PER_CHECK = {"dvq_vq_assign_nchw_f32": 8, "dvq_vq_assign_nchw_x16": 11, "dvq_vq_assign_flat_f32": 2, "dvq_vq_backward_nchw_f32": 5,
              "dvq_vq_backward_nchw_x16": 7, "dvq_ema_accumulate_nchw_f32": 2, "dvq_ema_accumulate_nchw_x16": 4, "dvq_vq_assign_qconv_f32": 11,
              "dvq_vq_assign_fold_f32": 10, "dvq_vq_assign_routed_dual_f32": 10, "dvq_vq_assign_routed_triple_f32": 11,
              "dvq_vq_soft_assign_flat_f32": 8, "dvq_vq_score_assign_f32": 8, "dvq_vq_apply_codes_nchw_f32": 8, "dvq_vq_apply_codes_flat_f32": 1,
              "dvq_gumbel_prepare_f32": 4, "dvq_vq_gumbel_assign_f32": 9, "dvq_vq_assign_narrow_nchw_f32": 8, "dvq_vq_assign_narrow_flat_f32": 9,
              "dvq_codebook_prepare_f32": 4, "dvq_fold_prepare_f32": 4, "dvq_router_gate_f32": 13}


def test_the_abi_refuses_what_it_refused_with_the_same_words():
    table = json.load(open(TABLE))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    out = subprocess.run([sys.executable, TOOL, "--replay", TABLE], env=env, check=True, capture_output=True, text=True, timeout=120).stdout
    got = json.loads(out)
    assert len(got) == len(table)
    for row, (rc, message) in zip(table, got):
        assert row["rc"] in (-1, -2, -3), row                 # the table holds refusals only
        assert (rc, message) == (row["rc"], row["message"]), (row["fn"], row["args"])


def test_the_table_covers_every_entry_point_and_the_checks_of_the_assign_family():
    import ctypes
    from dynamicvectorquantization_amd import _lib
    table = json.load(open(TABLE))
    checks = {}                                               # per entry point: its distinct messages, numbers aside
    for row in table:
        checks.setdefault(row["fn"], set()).add(re.sub(r"-?\d+", "#", row["message"]))
    refusing = {name for name, (ret, args) in _lib._PROTOTYPES.items() if ret is ctypes.c_int and args and name not in _lib._INT_QUERIES}
    assert set(checks) == refusing, set(checks) ^ refusing
    for fn, n in _PER_CHECK.items():
        assert len(checks[fn]) >= n, (fn, sorted(checks[fn]), n)
