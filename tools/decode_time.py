"""The decode head (csrc/decode_head.hip) against the torch-op chain the package offered before it.  CUDA events, median of
--iters after --warmup, the two forms alternating in one run.  At (B, C, K) = (256, 256, 1024) and (16, 256, 1024), 32 x 32,
position_type fourier+learned, from the token streams of a synthetic dual-grain batch:
  chain   permuter.forward_back (kernel) -> quantize.get_codebook_entry (`dvq_embed_gather_f32`) -> .permute(0, 3, 1, 2) ->
          F.conv2d (post_quant_conv) -> the decoder's own position modules
  fused   DecodeHead.from_tokens: forward_back, then `dvq_decode_head_f32`
  head    DecodeHead.from_codes alone (one launch; the host call included)
and the algorithmic bytes B * HW * (4 C + 8) over the kernel's time as a share of the 8 TB/s peak and of the ~6.3 TB/s a
streaming kernel reaches.  The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run of
`--profile-loop` (pass its stats CSV as --kernel-stats to merge the decode_head_kernel line).  Also: max |F_gpu - F_golden| of
the fourier table against tests/golden/decode_head_dual (the figure tests/test_decode.py asserts four times of), the outputs of
the two forms compared, and the resource table of the kernels (tools/kernel_resources.py).

    python tools/decode_time.py [--iters 30] [--warmup 5] [--out profiles/decode.json]
"""
import argparse
import csv
import json
import os
import subprocess
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd import _lib, synth  # noqa: E402
from dynamicvectorquantization_amd.decode import DecodeHead  # noqa: E402
from dynamicvectorquantization_amd.permuter import DualGrainSeperatePermuter  # noqa: E402
from dynamicvectorquantization_amd.quantize import VectorQuantize2  # noqa: E402
from tests import _decode_ref as R  # noqa: E402

PEAK, ACHIEVABLE = 8.0e12, 6.3e12


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternating_medians(fns, iters, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(iters):
        for k, fn in fns.items():
            ts[k].append(event_ms(fn))
    return {k: float(np.median(v)) for k, v in ts.items()}, {k: [float(min(v)), float(max(v))] for k, v in ts.items()}


def model(dev, K=1024, D=256, C=256, hw=32):
    S = R.stub_modules()
    torch.manual_seed(5)
    q = VectorQuantize2(K, D).to(dev).eval()
    conv = torch.nn.Conv2d(D, C, 1).to(dev).eval()
    with torch.no_grad():
        q.codebook.weight[:-1].copy_(torch.from_numpy(synth.codebook_trained(K, D)).to(dev))
        conv.weight.copy_(torch.from_numpy(synth.normal(9701, (C, D, 1, 1), 0.0, 1.0 / 16.0)).to(dev))
        conv.bias.copy_(torch.from_numpy(synth.normal(9702, (C,), 0.0, 0.1)).to(dev))
    dec = S.Decoder(C, hw, "fourier+learned").to(dev).eval()
    return q, conv, dec


def streams(dev, perm, B, K=1024):
    codes = torch.from_numpy(synth.randint(7000 + B, (B, 32, 32), K).astype(np.int64)).to(dev)
    grain = torch.from_numpy(synth.grain_gate_dual(7100 + B, B, 16, 16)).to(dev)
    if grain.dim() == 4:
        grain = grain.argmax(-1)
    out = perm(codes, grain.long())
    return [out[k] for k in ("coarse_content", "fine_content", "coarse_position", "fine_position")]


def delta_f(dev):
    g = R.load("decode_head_dual")
    S = R.stub_modules()
    dec = S.Decoder(256, 32, "fourier+learned").to(dev).eval()
    dec.load_state_dict({k[6:]: torch.from_numpy(g[k]) for k in g if k.startswith("param/")}, strict=False)
    head = DecodeHead(torch.nn.Embedding(4, 256).to(dev), None, dec)
    with torch.no_grad():
        Fg, Lg = [t.cpu().numpy().reshape(256, 32, 32) for t in head.position_tables(32, 32, dev)]
    return float(np.abs(Fg - g["pos_first"]).max()), bool(np.array_equal(Lg, g["pos_second"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "decode.json"))
    ap.add_argument("--profile-loop", type=int, default=0, help="only run from_tokens this many times at each size (for rocprofv3)")
    ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a rocprofv3 run of --profile-loop")
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "decode_time.py needs a GPU"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    q, conv, dec = model(dev)
    perm = DualGrainSeperatePermuter()
    head = DecodeHead(q, conv, dec)
    rec = {"device": torch.cuda.get_device_name(0), "library": os.path.basename(_lib.LIB_PATH), "label": args.label,
           "iters": args.iters, "warmup": args.warmup, "sizes": {}}
    for B in (256, 16):
        st = streams(dev, perm, B)

        def chain():
            idx = perm.forward_back(*st)
            h = conv(q.get_codebook_entry(idx).permute(0, 3, 1, 2))
            return dec.position_block(h)

        def fused():
            return head.from_tokens(perm, *st)

        if args.profile_loop:
            for _ in range(args.profile_loop):
                fused()
            torch.cuda.synchronize()
            continue
        idx = perm.forward_back(*st)
        a, b = chain(), fused()
        diff = float((a - b).abs().max())
        med, rng = alternating_medians({"chain": chain, "fused": fused, "head": lambda: head.from_codes(idx)}, args.iters, args.warmup)
        nbytes = B * 1024 * (4 * 256 + 8)
        size = {"chain_ms": med["chain"], "fused_ms": med["fused"], "head_ms": med["head"], "min_max_ms": rng,
                "speedup_fused_over_chain": med["chain"] / med["fused"], "max_abs_diff_chain_vs_fused": diff,
                "algorithmic_bytes": nbytes, "head_event_share_of_peak": nbytes / (med["head"] * 1e-3) / PEAK,
                "head_event_share_of_achievable": nbytes / (med["head"] * 1e-3) / ACHIEVABLE}
        rec["sizes"]["B%d" % B] = size
        print(json.dumps({"B": B, **size}))
    if args.profile_loop:
        return
    rec["delta_F_max_abs"], rec["learned_table_bit_equal_to_golden"] = delta_f(dev)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "decode_head.hip"],
                         capture_output=True, text=True).stdout
    rec["kernel_resources"] = [ln.strip() for ln in res.splitlines() if ln.strip()]
    if args.kernel_stats and os.path.exists(args.kernel_stats):
        for row in csv.DictReader(open(args.kernel_stats)):
            if "decode_head_kernel" in row.get("Name", ""):
                rec["kernel_trace"] = {k: row[k] for k in ("Name", "Calls", "AverageNs", "MinNs", "MaxNs") if k in row}
    print(json.dumps({k: rec[k] for k in ("delta_F_max_abs", "learned_table_bit_equal_to_golden")}))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
