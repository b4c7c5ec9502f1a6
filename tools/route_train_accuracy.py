"""Accuracy of the training-mode routing tail (route_train_dual / route_train_triple) at the ragged shapes of
tests/_route_train_ref.py: per row and tensor, the largest error of the kernels and of the package's fp32 torch-op chain against
the float64 statement of the op, their ratio, and the factor m that the slice rule of tests/test_route_train_shapes.py
(err_kernel <= m err_torch32 + 16 * 2^-24 * max |ref| on every slice) needs.  Both sides run on the GPU on the same inputs.

    python tools/route_train_accuracy.py [--out profiles/route_train_accuracy.json] [--commit <hash>]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import _route_train_ref as R  # noqa: E402


def _finite(x):
    """json has no inf: a ratio over an exact fp32 chain is written as the string 'inf'"""
    if isinstance(x, dict):
        return {k: _finite(v) for k, v in x.items()}
    return "inf" if isinstance(x, float) and x == float("inf") else x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "route_train_accuracy.json"))
    ap.add_argument("--commit", default="unknown", help="the commit whose kernels are measured (recorded as given)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows, worst = {}, {}
    for i in list(range(len(R.CASES))) + [-1]:
        inp, ref = R.case(i)
        ker, t32 = R.run_kernel(inp, dev), R.run_torch32(inp, dev)
        same = torch.equal(ker["indices"].cpu(), ref["indices"]) and torch.equal(t32["indices"].cpu(), ref["indices"])
        rec = R.accuracy_record(inp, ref, ker, t32)
        name = R.case_id(inp.row) + ("" if inp.update_router else "-no-update")
        rows[name] = {"cells": inp.geo["N"], "decisions_equal_float64": same, "tensors": rec}
        for t, r in rec.items():
            worst[t] = max(worst.get(t, 0.0), r["m_needed"])
        print("%-58s m_needed %.3g" % (name, max(r["m_needed"] for r in rec.values())))
    out = {"tool": "tools/route_train_accuracy.py", "commit": args.commit, "device": torch.cuda.get_device_name(0),
           "floor_roundings": R.FLOOR_ROUNDINGS, "worst_m_needed_per_tensor": worst, "rows": rows}
    with open(args.out, "w") as f:
        json.dump(_finite(out), f, indent=1, sort_keys=True)
        f.write("\n")
    print("worst m needed: %.3g -> %s" % (max(worst.values()), args.out))


if __name__ == "__main__":
    main()
