"""Forward + backward of the training-mode routing tail: route_train_dual / route_train_triple (one op, dvq_route_train_*_f32)
against the torch-op path it replaces (the router module's training forward, F.gumbel_softmax, argmax / repeat_interleave /
where / * gate_grad), group-32 + 2layer-fc-SiLu as in the stage-1 configs, C = 256.  Loss sum(h_out * R) + sum(gate * Q).
Shapes: dual coarse 16 x 16 (fine 32 x 32), triple coarse 8 x 8 (fine 32 x 32), each at B = 30 (the recipe's per-GPU batch)
and B = 256.  Median of --iters CUDA-event timings after --warmup; one JSON line per shape, and the whole record to --out if given.

    python tools/route_train_time.py [--iters 30] [--warmup 5] [--only op] [--out record.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd.router import (DualGrainFeatureRouter, TripleGrainFeatureRouter,  # noqa: E402
                                                  route_train_dual, route_train_triple)


def torch_path(router, hs, nb):
    if nb == 2:
        gate = router(h_fine=hs[1], h_coarse=hs[0])
    else:
        gate = router(h_fine=hs[2], h_median=hs[1], h_coarse=hs[0])
    gate = F.gumbel_softmax(gate, tau=1, dim=-1, hard=True).permute(0, 3, 1, 2)
    indices = gate.argmax(dim=1)
    S = 2 if nb == 2 else 4
    rep = lambda t, s: t.repeat_interleave(s, dim=-1).repeat_interleave(s, dim=-2)
    ir = rep(indices, S).unsqueeze(1)
    if nb == 2:
        h = torch.where(ir == 0, rep(hs[0], 2), hs[1])
    else:
        hm = rep(hs[1], 2)
        h = torch.where(ir == 0, rep(hs[0], 4), hm)
        h = torch.where(ir == 1, hm, h)
        h = torch.where(ir == 2, hs[2], h)
    h = h * rep(gate.max(dim=1, keepdim=True)[0], S)
    return h, gate


def op_path(router, hs, nb):
    if nb == 2:
        out = route_train_dual(router, hs[1], hs[0])
        return out["h_dual"], out["gate"]
    out = route_train_triple(router, hs[2], hs[1], hs[0])
    return out["h_triple"], out["gate"]


def time_one(fn, router, hs, nb, R, Q, iters, warmup):
    params = list(router.parameters())

    def step():
        h, gate = fn(router, hs, nb)
        torch.autograd.grad((h * R).sum() + (gate * Q).sum(), hs + params)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return {"median_us": ts[len(ts) // 2], "min_us": ts[0], "max_us": ts[-1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", choices=["op", "torch"], default=None)
    ap.add_argument("--out", default=None, help="write the record (device name + rows) to this JSON file")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for nb, hc in ((2, 16), (3, 8)):
        for B in (30, 256):
            torch.manual_seed(0)
            C = 256
            cls = DualGrainFeatureRouter if nb == 2 else TripleGrainFeatureRouter
            router = cls(C, normalization_type="group-32", gate_type="2layer-fc-SiLu").to(dev)
            hs = [torch.randn((B, C, hc * s, hc * s), device=dev).requires_grad_(True)
                  for s in ((1, 2) if nb == 2 else (1, 2, 4))]
            S = 2 if nb == 2 else 4
            R = torch.randn((B, C, S * hc, S * hc), device=dev)
            Q = torch.randn((B, nb, hc, hc), device=dev)
            row = {"nb": nb, "B": B, "C": C, "hc": hc}
            if args.only != "op":
                row["torch_ops"] = time_one(torch_path, router, hs, nb, R, Q, args.iters, args.warmup)
            if args.only != "torch":
                row["route_train"] = time_one(op_path, router, hs, nb, R, Q, args.iters, args.warmup)
            if "torch_ops" in row and "route_train" in row:
                row["speedup"] = row["torch_ops"]["median_us"] / row["route_train"]["median_us"]
            rows.append(row)
            print(json.dumps(row), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
