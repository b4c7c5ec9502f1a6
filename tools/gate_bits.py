#!/usr/bin/env python3
"""sha256 of the feature-router gate's logits over every row of tests/_gate_ref.CASES, to show that a change of csrc/router_gate.hip
which only moves code left every bit of its output as it was: run once per library (DVQ_LIBRARY=<the other build's libdvq.so>) and
compare the two JSON lines with cmp -- the line does not name the library, so equal bits give equal lines.

Per row, on the row's own seeded inputs (tests/_gate_ref.Inputs):
  features   float32, float16, bfloat16 (the float32 values rounded)
  layout     NCHW, channels_last
  prep       kept  -- the module's call: weight images kept by dvq_router_gate_prepare_f32 + ..._prepare_norm_f32, so the pooling
                      pass takes the fp16 range bound from the prepared GroupNorm maxima
             built -- fused_router_gate without a weight prep: images rebuilt inside the call, the pooling pass scans the parameters
"""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dynamicvectorquantization_amd.router import fused_router_gate  # noqa: E402
from tests import _gate_ref as G  # noqa: E402


def main():
    dev = torch.device("cuda:0")
    out = {}
    for case in G.CASES:
        inp = G.Inputs(case)
        router, hs32 = G.on(inp, dev)
        norms = [router.feature_norm_coarse] + ([router.feature_norm_median] if inp.nb == 3 else []) + [router.feature_norm_fine]
        for tname, dt in (("f32", torch.float32), ("f16", torch.float16), ("bf16", torch.bfloat16)):
            for lname, fmt in (("nchw", torch.contiguous_format), ("nhwc", torch.channels_last)):
                hs = [h.to(dt).contiguous(memory_format=fmt) for h in hs32]
                with torch.no_grad():
                    got = {"kept": G.run_kernel(inp, dev, router, hs),
                           "built": fused_router_gate(router.gate, router.gate_type, norms, hs, weight_prep=None)}
                for pname, t in got.items():
                    assert t.dtype == torch.float32 and tuple(t.shape) == tuple(inp.logits64.shape)
                    out["%s/%s/%s/%s" % (case[0], tname, lname, pname)] = hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()
        del router, hs32, hs, got
    print("library:", os.environ.get("DVQ_LIBRARY", "this build's"), file=sys.stderr)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
