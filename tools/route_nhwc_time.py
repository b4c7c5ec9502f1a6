#!/usr/bin/env python3
"""channels_last branch features through the routing tail: this build against the parent commit -> profiles/route_nhwc.json.

  tools/route_nhwc_time.py --parent-root <checkout of the parent commit, library built> [-o profiles/route_nhwc.json] [--bench]
      runs, one fresh process each and in this order, parent / this build / parent / this build, each under its own time limit;
      the two parent runs give the parent's own run-to-run spread, and a row is marked slower when this build's time is more than
      that spread above the parent's.
      --bench: afterwards one plain `bench.py --gpus 1 --steps 200 --warmup 20` of each checkout and a second one of the parent
      (the float32 headline, which runs none of this code), recorded under "bench" with the parent's own spread.
  tools/route_nhwc_time.py --measure [--root <checkout>]
      one process: measures every row with the package it finds in --root (default: this checkout) and prints one JSON line.
  tools/route_nhwc_time.py --gate-workload dual|triple
      the workload of a `rocprofv3 --kernel-trace --stats` run of its own: the gate on channels_last tensors and on their NCHW copies,
      float32 and bfloat16, 20 calls each (per-kernel times of the two pooling passes, gate_pool_rows_kernel / gate_pool_kernel).
  tools/route_nhwc_time.py --pool-table <dir of such a run's csv> ...
      the pooling kernels' average times and achieved bytes/s from the kernel-stats CSVs.

BOTH builds receive the same channels_last tensors, as a channels_last encoder leaves them.  The parent's side of a row is what
its caller has today -- the same function, which copies every branch to NCHW inside and returns NCHW; this build's side reads them
in place.  Per row: HIP events around every call, 5 warm-ups, the median of 30 (B >= 64) or 100 calls in microseconds.
  select_dual_B256_{f32,bf16}   route_select_dual, int64 gate, features [256, 256, 16, 16] / [256, 256, 32, 32]
  gate_dual_B64_{f32,bf16}      DualGrainFeatureRouter(256, group-32, 2layer-fc-SiLu), no grad, fine [64, 256, 32, 32]
  gate_triple_B128_{f32,bf16}   TripleGrainFeatureRouter(256, group-32, 2layer-fc-SiLu), no grad, fine [128, 256, 32, 32]
  encode_dual_bf16_B*[_conv]    encode_dual, fixed-entropy router, eval VectorQuantize2(1024, 256), fine [B, 256, 32, 32], without and
                                with a channels_last 1x1 quant_conv
  encode_dual_f32_B256_fused    float32: encode_dual as it dispatches (the fused routed op, which copies to NCHW inside), and
  encode_dual_f32_B256_chain    the chain select -> quantizer composed by hand, channels_last end to end in this build: which of
                                the two float32 callers should take is decided by these two figures in a later change, not here
"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _setup(root):
    sys.path.insert(0, root)
    import torch
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(7)
    cl = torch.channels_last
    feat = lambda B, s, dt: torch.randn(B, 256, s, s, device=dev, generator=g).to(dt).contiguous(memory_format=cl)
    return torch, dev, feat


def measure(root):
    torch, dev, feat = _setup(root)
    from dynamicvectorquantization_amd import _lib, synth
    from dynamicvectorquantization_amd.encode import encode_dual
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    from dynamicvectorquantization_amd.router import (DualGrainFeatureRouter, DualGrainFixedEntropyRouter, TripleGrainFeatureRouter,
                                                      route_select_dual, route_select_dual_entropy)
    rows = {}

    def timed(fn, reps):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for s, t in ev:
            s.record()
            fn()
            t.record()
        torch.cuda.synchronize()
        return round(statistics.median(s.elapsed_time(t) for s, t in ev) * 1e3, 1)

    with torch.no_grad():
        rd = DualGrainFeatureRouter(256, "group-32", "2layer-fc-SiLu").to(dev).eval()
        rt = TripleGrainFeatureRouter(256, "group-32", "2layer-fc-SiLu").to(dev).eval()
        K, D = 1024, 256
        vq = VectorQuantize2(K, D).to(dev).eval()
        vq.codebook.weight.data[:-1].copy_(torch.from_numpy(synth.codebook_trained(K, D)).to(dev))
        fixed = DualGrainFixedEntropyRouter(os.path.join(root, "tests", "golden", "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
        gate = torch.from_numpy(synth.grain_gate_dual(11, 256, 16, 16)).to(dev)
        for name, dt in (("f32", torch.float32), ("bf16", torch.bfloat16)):
            hf, hc = feat(256, 32, dt), feat(256, 16, dt)
            sel = lambda: route_select_dual(gate, hc, hf)["h_dual"]
            want = torch.where(gate.argmax(-1).repeat_interleave(2, 1).repeat_interleave(2, 2).unsqueeze(1) == 1, hf,
                               hc.repeat_interleave(2, 2).repeat_interleave(2, 3))
            assert torch.equal(sel(), want), "select differs from the torch expression"
            del want
            rows["select_dual_B256_" + name] = timed(sel, 30)
            h64f, h64c = hf[:64], hc[:64]
            rows["gate_dual_B64_" + name] = timed(lambda: rd(h_fine=h64f, h_coarse=h64c), 30)
            t_f, t_m, t_c = hf[:128], hc[:128], feat(128, 8, dt)
            rows["gate_triple_B128_" + name] = timed(lambda: rt(h_fine=t_f, h_median=t_m, h_coarse=t_c), 30)
            if dt == torch.bfloat16:
                conv = torch.nn.Conv2d(D, D, 1).to(dev).eval().to(dt).to(memory_format=torch.channels_last)
                for B in (4, 256):
                    ef, ec = hf[:B], hc[:B]
                    ent = torch.from_numpy(synth.entropy_map(13, B, 16, 16)).to(dev)
                    for tag, c in (("", None), ("_conv", conv)):
                        enc = lambda: encode_dual(fixed, vq, ef, ec, entropy=ent, quant_conv=c)[0]
                        assert enc().dtype == dt
                        rows["encode_dual_bf16_B%d%s" % (B, tag)] = timed(enc, 30 if B >= 64 else 100)
            else:
                ent = torch.from_numpy(synth.entropy_map(13, 256, 16, 16)).to(dev)
                rows["encode_dual_f32_B256_fused"] = timed(lambda: encode_dual(fixed, vq, hf, hc, entropy=ent)[0], 30)

                def chain():
                    s = route_select_dual_entropy(ent, fixed.fine_grain_threshold, hc, hf)
                    return vq(x=s["h_dual"], codebook_mask=s["codebook_mask"])[0]
                rows["encode_dual_f32_B256_chain"] = timed(chain, 30)
            del hf, hc
    return {"abi": _lib.lib.dvq_version(), "rows": rows}


def gate_workload(which):
    torch, dev, feat = _setup(ROOT)
    from dynamicvectorquantization_amd.router import DualGrainFeatureRouter, TripleGrainFeatureRouter
    with torch.no_grad():
        if which == "dual":
            r, B = DualGrainFeatureRouter(256, "group-32", "2layer-fc-SiLu").to(dev).eval(), 64
        else:
            r, B = TripleGrainFeatureRouter(256, "group-32", "2layer-fc-SiLu").to(dev).eval(), 128
        for dt in (torch.float32, torch.bfloat16):
            hs = [feat(B, 32, dt), feat(B, 16, dt)] + ([feat(B, 8, dt)] if which == "triple" else [])
            for tensors in (hs, [h.contiguous() for h in hs]):
                kw = dict(h_fine=tensors[0], h_coarse=tensors[-1])
                if which == "triple":
                    kw["h_median"] = tensors[1]
                for _ in range(20):
                    r(**kw)
        torch.cuda.synchronize()


def pool_table(dirs):
    """{run: {kernel: (calls, average us, GB/s of feature bytes read)}} of the pooling kernels in rocprofv3 kernel-stats CSVs named
    .../<dual|triple>/..._kernel_stats.csv"""
    out = {}
    for d in dirs:
        which = "triple" if "triple" in os.path.basename(os.path.normpath(d)) else "dual"
        B = 128 if which == "triple" else 64
        elems = B * 256 * (32 * 32 + 16 * 16 + (8 * 8 if which == "triple" else 0))
        for f in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
            for r in csv.DictReader(open(f)):
                n = r["Name"]
                if "gate_pool" not in n:
                    continue
                m = re.search(r"gate_pool\w*<\w+, \w+(?:, (\d))?>", n)        # <IMG, NT[, XT]>: XT 0 (or absent) = float32
                es = 2 if (m and m.group(1) not in (None, "0")) else 4
                us = float(r["AverageNs"]) / 1e3
                out.setdefault(which, {})[n] = {"calls": int(r["Calls"]), "average_us": round(us, 2),
                                                 "feature_GB_per_s": round(elems * es / us / 1e3, 1)}
    return out


def bench(root):
    p = subprocess.run(["timeout", "-k", "10", "600", sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "200",
                        "--warmup", "20"], cwd=root, check=True, capture_output=True, text=True)
    line = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    return {k: v for k, v in line.items() if not isinstance(v, (dict, list))}          # the headline: metric, value, ms_per_step, ...


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--gate-workload", choices=("dual", "triple"))
    ap.add_argument("--pool-table", nargs="+")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "route_nhwc.json"))
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(os.path.abspath(a.root))))
        return
    if a.gate_workload:
        gate_workload(a.gate_workload)
        return
    if a.pool_table:
        print(json.dumps(pool_table(a.pool_table), indent=1))
        return
    if not a.parent_root:
        ap.error("--parent-root: a checkout of the parent commit with its library built")
    runs = []
    for which, root in (("parent", a.parent_root), ("this", ROOT)) * 2:       # each step under its own limit; a failure ends the run
        p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--measure", "--root",
                            os.path.abspath(root)], check=True, capture_output=True, text=True)
        runs.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), build=which))
        print(which, runs[-1]["rows"], flush=True)
    pa, ta, pb, tb = (r["rows"] for r in runs)
    table = {}
    for k in pa:
        spread = abs(pa[k] - pb[k])
        parent, this = (pa[k] + pb[k]) / 2, (ta[k] + tb[k]) / 2
        table[k] = {"parent_copying_us": [pa[k], pb[k]], "this_in_place_us": [ta[k], tb[k]], "parent_spread_us": round(spread, 1),
                    "speedup": round(parent / this, 2), "slower_than_parent_plus_spread": bool(this > parent + spread)}
    doc = {"tool": "tools/route_nhwc_time.py", "layout": "channels_last on both sides", "order": [r["build"] for r in runs],
           "abi": [r["abi"] for r in runs], "rows": table}
    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
        with open(a.o, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")

    write()
    print(json.dumps(table, indent=1), flush=True)
    if a.bench:
        doc["bench"] = {}
        for which, root in (("parent", a.parent_root), ("this", ROOT), ("parent_again", a.parent_root)):
            line = bench(os.path.abspath(root))
            doc["bench"][which] = line
            print("bench", which, json.dumps(line)[:300], flush=True)
            write()


if __name__ == "__main__":
    main()
