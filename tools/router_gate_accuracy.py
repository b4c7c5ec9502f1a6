"""Accuracy of the fused feature-router gate (fused_router_gate / dvq_router_gate_f32) at the rows of tests/_gate_ref.py: per row
and image, the largest error of the kernel and of the module's own fp32 torch-op forward against the float64 statement of the
routers, their ratio, and the factor m that the rule of tests/test_router_gate_shapes.py
(err_kernel <= m err_torch32 + 16 * 2^-24 * max |ref| on every image) needs.  Both sides run on the GPU on the same inputs; the
yardstick is the fp32 torch chain, never the kernel's own output.

    python tools/router_gate_accuracy.py [--out profiles/router_gate_accuracy.json] [--commit <hash>]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _gate_ref as G  # noqa: E402


def _finite(x):
    """json has no inf: a ratio over an exact fp32 chain is written as the string 'inf'"""
    if isinstance(x, dict):
        return {k: _finite(v) for k, v in x.items()}
    if isinstance(x, list):
        return [_finite(v) for v in x]
    return "inf" if isinstance(x, float) and x == float("inf") else x


def form_of(d):
    if d["gemm_form"]:
        return "gemm<%d,%d>%s" % (d["nb"], d["S16"], " PIPE" if d["PIPE"] else "")
    if d["act"] == 0:
        return "direct, single Linear"
    return "direct<%d,%d>%s" % (d["nb"], 2 if d["cb2"] else 1, "" if d["pipelined"] else " untiled")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "router_gate_accuracy.json"))
    ap.add_argument("--commit", default="unknown", help="the commit whose kernels are measured (recorded as given)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    rows, per_form, worst = {}, {}, 0.0
    for name in G.NAMES:
        inp = G.Inputs(G.row(name))                          # not kept: the largest rows hold 80 MB each
        d = G.dispatch(inp.case, ncu)
        router, hs = G.on(inp, dev)
        got, t32 = G.run_kernel(inp, dev, router, hs), G.run_torch32(inp, dev, router, hs)
        rec = G.accuracy_record(got, t32, inp.logits64)
        clear = G.clear_cells(inp.logits64, *G.image_errors(got, t32, inp.logits64)[1:])
        same = bool((got.cpu().argmax(-1) == inp.logits64.argmax(-1))[clear].all())
        if d["B"] > 8:                                       # per image figures of the large rows: the eight worst images
            order = sorted(range(d["B"]), key=lambda b: -rec["m_needed"][b])[:8]
            rec = dict({k: [v[b] for b in order] for k, v in rec.items() if isinstance(v, list)}, images=order,
                       worst_m_needed=rec["worst_m_needed"])
        form = form_of(d)
        rows[name] = {"edge": inp.case[-1], "form": form, "cells": d["ncell"], "cells_under_margin": int((~clear).sum()),
                      "argmax_equal_float64_on_clear_cells": same, "in_the_rule": name != G.ROW_OFFSET, "per_image": rec}
        if name != G.ROW_OFFSET:
            per_form[form] = max(per_form.get(form, 0.0), rec["worst_m_needed"])
            worst = max(worst, rec["worst_m_needed"])
        print("%-5s %-24s m_needed %.3g" % (name, form, rec["worst_m_needed"]), flush=True)
    out = {"tool": "tools/router_gate_accuracy.py", "commit": args.commit, "device": torch.cuda.get_device_name(0), "cus": ncu,
           "floor_roundings": G.FLOOR_ROUNDINGS, "M_of_the_tests": G.M, "worst_m_needed_rule_rows": worst,
           "worst_m_needed_per_form": per_form, "m_needed_offset_row": rows[G.ROW_OFFSET]["per_image"]["worst_m_needed"], "rows": rows}
    with open(args.out, "w") as f:
        json.dump(_finite(out), f, indent=1, sort_keys=True)
        f.write("\n")
    print("worst m needed over the rule's rows: %.3g -> %s" % (worst, args.out))


if __name__ == "__main__":
    main()
