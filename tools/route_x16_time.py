#!/usr/bin/env python3
"""bf16 branch features through the routing tail: this build against the parent commit -> profiles/route_x16.json.

  tools/route_x16_time.py --parent-root <checkout of the parent commit, library built> [-o profiles/route_x16.json] [--bench]
      runs, one fresh process each and in this order, parent / this build / parent / this build; the two parent runs give the
      parent's own run-to-run spread, and a row PASSES when this build's time is no more than that spread above the parent's.
      --bench: afterwards one plain `bench.py --gpus 1 --steps 200 --warmup 20` of each checkout (the float32 headline, which runs
      none of this code), recorded under "bench".
  tools/route_x16_time.py --measure
      one process: measures every row with the package it finds in --root (default: this checkout) and prints one JSON line.

The features are bfloat16 on the GPU in both builds, as an encoder under autocast leaves them.  The PARENT's side of a row is the
only way its caller has: `.float()` on every feature map -> the float32 op -> `.to(torch.bfloat16)` on the feature-shaped result
(h_dual, quant); the gate's logits are float32 either way, so its rows cast on the way in only.  THIS build's side passes the
bfloat16 tensors to the same Python function.  Per row: HIP events around every call, 5 warm-ups, the median of 30 (B >= 64) or
100 calls in microseconds.
  select_dual_B256          route_select_dual, int64 gate, features [256, 256, 16, 16] / [256, 256, 32, 32]
  gate_dual_B64             DualGrainFeatureRouter(256, group-32, 2layer-fc-SiLu), no grad, fine [64, 256, 32, 32]
  gate_triple_B128          TripleGrainFeatureRouter(256, group-32, 2layer-fc-SiLu), no grad, fine [128, 256, 32, 32]
  encode_dual_B*[_conv]     encode_dual, fixed-entropy router, eval VectorQuantize2(1024, 256), fine [B, 256, 32, 32], without and
                            with a 1x1 quant_conv (parent: the fused routed op, float32 conv; this build: select -> torch conv in
                            bfloat16 -> dense 16-bit assign)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(root):
    sys.path.insert(0, root)
    import torch
    from dynamicvectorquantization_amd import _lib, synth
    from dynamicvectorquantization_amd.encode import encode_dual
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    from dynamicvectorquantization_amd.router import (DualGrainFeatureRouter, DualGrainFixedEntropyRouter, TripleGrainFeatureRouter,
                                                      route_select_dual)
    dev = torch.device("cuda:0")
    dt = torch.bfloat16
    new = _lib.lib.dvq_version() >= 1900                  # ABI 0.19.0: DVQ_FEATURES
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

    g = torch.Generator(device=dev).manual_seed(7)
    feat = lambda B, s: torch.randn(B, 256, s, s, device=dev, generator=g).to(dt)
    with torch.no_grad():
        B = 256
        hf, hc = feat(B, 32), feat(B, 16)
        gate = torch.from_numpy(synth.grain_gate_dual(11, B, 16, 16)).to(dev)
        if new:
            sel = lambda: route_select_dual(gate, hc, hf)["h_dual"]
        else:
            sel = lambda: route_select_dual(gate, hc.float(), hf.float())["h_dual"].to(dt)
        want = torch.where(gate.argmax(-1).repeat_interleave(2, 1).repeat_interleave(2, 2).unsqueeze(1) == 1, hf,
                           hc.repeat_interleave(2, 2).repeat_interleave(2, 3))
        assert torch.equal(sel(), want), "select differs from the torch expression"
        rows["select_dual_B256"] = timed(sel, 30)
        del want

        rd = DualGrainFeatureRouter(256, "group-32", "2layer-fc-SiLu").to(dev).eval()
        h64f, h64c = hf[:64], hc[:64]
        if new:
            gd = lambda: rd(h_fine=h64f, h_coarse=h64c)
        else:
            gd = lambda: rd(h_fine=h64f.float(), h_coarse=h64c.float())
        rows["gate_dual_B64"] = timed(gd, 30)
        rt = TripleGrainFeatureRouter(256, "group-32", "2layer-fc-SiLu").to(dev).eval()
        t_f, t_m, t_c = hf[:128], hc[:128], feat(128, 8)
        if new:
            gt = lambda: rt(h_fine=t_f, h_median=t_m, h_coarse=t_c)
        else:
            gt = lambda: rt(h_fine=t_f.float(), h_median=t_m.float(), h_coarse=t_c.float())
        rows["gate_triple_B128"] = timed(gt, 30)

        K, D = 1024, 256
        vq = VectorQuantize2(K, D).to(dev).eval()
        vq.codebook.weight.data[:-1].copy_(torch.from_numpy(synth.codebook_trained(K, D)).to(dev))
        fixed = DualGrainFixedEntropyRouter(os.path.join(root, "tests", "golden", "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
        conv32 = torch.nn.Conv2d(D, D, 1).to(dev).eval()
        conv16 = torch.nn.Conv2d(D, D, 1).to(dev).eval().to(dt)
        conv16.load_state_dict({k: v.to(dt) for k, v in conv32.state_dict().items()})
        for B in (4, 256):
            ef, ec = hf[:B], hc[:B]
            ent = torch.from_numpy(synth.entropy_map(13, B, 16, 16)).to(dev)
            for name, c32, c16 in (("", None, None), ("_conv", conv32, conv16)):
                if new:
                    enc = lambda: encode_dual(fixed, vq, ef, ec, entropy=ent, quant_conv=c16)[0]
                else:
                    enc = lambda: encode_dual(fixed, vq, ef.float(), ec.float(), entropy=ent, quant_conv=c32)[0].to(dt)
                assert enc().dtype == dt
                rows["encode_dual_B%d%s" % (B, name)] = timed(enc, 30 if B >= 64 else 100)
    return {"abi": _lib.lib.dvq_version(), "dtype": "bfloat16", "rows": rows}


def bench(root):
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "200", "--warmup", "20"], cwd=root,
                       check=True, capture_output=True, text=True, timeout=900)
    line = json.loads([l for l in p.stdout.strip().splitlines() if l.startswith("{")][-1])
    return {k: v for k, v in line.items() if not isinstance(v, (dict, list))}          # the headline: metric, value, ms_per_step, ...


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--measure", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--parent-root")
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("-o", default=os.path.join(ROOT, "profiles", "route_x16.json"))
    a = ap.parse_args()
    if a.measure:
        print(json.dumps(measure(os.path.abspath(a.root))))
        return
    if not a.parent_root:
        ap.error("--parent-root: a checkout of the parent commit with its library built")
    runs = []
    for which, root in (("parent", a.parent_root), ("this", ROOT)) * 2:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--measure", "--root", os.path.abspath(root)], check=True,
                           capture_output=True, text=True, timeout=600)
        runs.append(dict(json.loads(p.stdout.strip().splitlines()[-1]), build=which))
        print(which, runs[-1]["rows"], flush=True)
    pa, ta, pb, tb = (r["rows"] for r in runs)
    table = {}
    for k in pa:
        spread = abs(pa[k] - pb[k])
        parent, this = (pa[k] + pb[k]) / 2, (ta[k] + tb[k]) / 2
        table[k] = {"parent_cast_route_us": [pa[k], pb[k]], "this_16bit_us": [ta[k], tb[k]], "parent_spread_us": round(spread, 1),
                    "speedup": round(parent / this, 2), "not_slower_than_parent_plus_spread": bool(this <= parent + spread)}
    doc = {"tool": "tools/route_x16_time.py", "dtype": "bfloat16", "order": [r["build"] for r in runs], "abi": [r["abi"] for r in runs],
           "rows": table}
    if a.bench:
        doc["bench"] = {}
        for which, root in (("parent", a.parent_root), ("this", ROOT)):
            line = bench(os.path.abspath(root))
            doc["bench"][which] = line
            print("bench", which, json.dumps(line)[:300], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(table, indent=1))


if __name__ == "__main__":
    main()
