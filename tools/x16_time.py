"""16-bit latents (dvq_*_x16) against what a caller had to write before them: `x.float()` -> the float32
op -> `.to(dtype)`.  HIP events, median of --iters after --warmup, one process, B = 256, 32 x 32, D = 256, K = 1024.  Cases, per dtype:
  assign   eval-mode VectorQuantize2 forward (codes, loss, x_q)
  train    training-mode forward (EMA step, no restarts) + backward to x of sum(x_q * g) + loss
`x16` takes the 16-bit tensor as it is; `cast` is the parent-equivalent sequence on the same module.  One JSON line per case, the
whole record to --out.  No ratio is a condition of anything: the numbers are a measurement.

    python tools/x16_time.py [--iters 20] [--warmup 5] [--batch 256] [--out profiles/x16.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd import synth  # noqa: E402
from dynamicvectorquantization_amd.quantize import VectorQuantize2  # noqa: E402


def median_ms(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "x16.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    B, K, D, H, W = args.batch, 1024, 256, 32, 32
    E = synth.codebook_trained(K, D)
    x32 = torch.from_numpy(synth.z_tokens(E, B, H, W, 4101)).to(dev)
    g32 = torch.from_numpy(synth.normal(4102, (B, D, H, W))).to(dev)
    record = dict(device=torch.cuda.get_device_name(0), B=B, K=K, D=D, H=H, W=W, iters=args.iters, warmup=args.warmup, cases=[])

    def module(train):
        m = VectorQuantize2(K, D, restart_unused_codes=False).to(dev)
        m.codebook.weight.data[:-1].copy_(torch.from_numpy(E))
        m.codebook.embed_ema.copy_(torch.from_numpy(E))
        m.codebook.cluster_size_ema.fill_(float(B * H * W) / K)
        return m.train() if train else m.eval()

    for name, dtype in (("bf16", torch.bfloat16), ("f16", torch.float16)):
        x16, g16 = x32.to(dtype), g32.to(dtype)
        ev = module(False)

        def assign_x16():
            with torch.no_grad():
                return ev(x16)

        def assign_cast():
            with torch.no_grad():
                xq, loss, info = ev(x16.float())
                return xq.to(dtype), loss, info

        a, b = assign_x16(), assign_cast()
        torch.cuda.synchronize()
        assert torch.equal(a[2][2], b[2][2]) and torch.equal(a[0].view(torch.int16), b[0].view(torch.int16))
        tr = module(True)

        def train_x16():
            x = x16.detach().requires_grad_(True)
            xq, loss, _ = tr(x)
            ((xq * g16).sum(dtype=torch.float32) + loss).backward()
            return x.grad

        def train_cast():
            x = x16.detach().requires_grad_(True)
            xq, loss, _ = tr(x.float())
            ((xq.to(dtype) * g16).sum(dtype=torch.float32) + loss).backward()
            return x.grad

        for case, f16, fc in (("assign", assign_x16, assign_cast), ("train", train_x16, train_cast)):
            t16, tc = median_ms(f16, args.iters, args.warmup), median_ms(fc, args.iters, args.warmup)
            row = dict(case=case, dtype=name, x16_ms=round(t16, 4), cast_ms=round(tc, 4), cast_over_x16=round(tc / t16, 3))
            record["cases"].append(row)
            print(json.dumps(row))
    with open(args.out, "w") as f:
        json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
