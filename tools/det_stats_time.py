#!/usr/bin/env python3
"""The fixed-order per-code sums (dvq_code_sums_det, dvq_vq_backward_codebook_det_f32) against the float-atomic kernels of the same
build, one process, HIP events: per shape 5 warm-up calls of each, then 20 timed calls of each, the two ALTERNATING (so that a drift
of the clocks or of a neighbour's load falls on both), median and spread reported.  Also a VectorQuantize2 training step (forward,
backward, EMA update) with the switch on and off.

  tools/det_stats_time.py [-o profiles/det_stats.json] [--reps 20] [--warmup 5]
  rocprofv3 --kernel-trace --stats -d <dir> -o t --output-format csv -- python3 tools/det_stats_time.py --calls-only 20
      the per-kernel split of the three launches (det_sort_kernel, det_partial_kernel, det_reduce_kernel) beside the atomic kernels

Results are checked as they are timed: counts equal, sums within 1e-5 of the largest entry of each other."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dynamicvectorquantization_amd as pkg  # noqa: E402
from dynamicvectorquantization_amd import _lib  # noqa: E402
from dynamicvectorquantization_amd.quantize import VectorQuantize2  # noqa: E402


def timed(fns, reps, warmup):
    """{name: [us per call]} of the callables, alternating"""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    out = {n: [] for n in fns}
    for _ in range(reps):
        for n, f in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            out[n].append(e0.elapsed_time(e1) * 1e3)
    return out


def summary(us):
    s = sorted(us)
    return {"median_us": round(statistics.median(s), 1), "min_us": round(s[0], 1), "max_us": round(s[-1], 1)}


def code_patterns(B, HW, K, dev, g):
    side = int(HW ** 0.5)
    fine = torch.randint(0, K, (B, side, side), device=dev, generator=g)
    up = lambda x: x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    pick = lambda p: torch.rand((B, side, side), device=dev, generator=g) < p
    coarse = up(torch.randint(0, K, (B, side // 2, side // 2), device=dev, generator=g))
    return {"uniform": fine,
            "dual_grain": torch.where(up(torch.rand((B, side // 2, side // 2), device=dev, generator=g) < 0.5), coarse, fine).contiguous(),
            "hot_code_10pct": torch.where(pick(0.1), torch.zeros_like(fine), fine).contiguous(),
            "hot_code_50pct": torch.where(pick(0.5), torch.full_like(fine, 7), fine).contiguous()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", default=os.path.join("profiles", "det_stats.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--calls-only", type=int, default=0, metavar="N",
                    help="no timing: N calls of each form at the first shape (uniform codes), for a run under rocprofv3 --kernel-trace --stats")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU: there is no CPU timing"
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    B, D, side, K = a.batch, 256, 32, 1024
    HW = side * side
    z32 = torch.randn(B, D, side, side, device=dev, generator=g)
    rows = []

    def stats_case(label, z, codes, Bz, Dz, HWz, Kz):
        x16 = _lib.X16.get(z.dtype, 0)
        cs = [torch.empty(Kz, device=dev) for _ in range(2)]
        vs = [torch.empty(Kz, Dz, device=dev) for _ in range(2)]
        ws = _lib.det_workspace(Bz, Dz, HWz, Kz, dev)
        st = _lib.stream_ptr(dev)

        def atomic():
            if x16:
                _lib.checked.dvq_ema_accumulate_nchw_x16(z.data_ptr(), x16, codes.data_ptr(), Bz, Dz, HWz, Kz, cs[0].data_ptr(), vs[0].data_ptr(), st)
            else:
                _lib.checked.dvq_ema_accumulate_nchw_f32(z.data_ptr(), codes.data_ptr(), Bz, Dz, HWz, Kz, cs[0].data_ptr(), vs[0].data_ptr(), st)

        def det():
            _lib.checked.dvq_code_sums_det(z.data_ptr(), x16, codes.data_ptr(), Bz, Dz, HWz, Kz, cs[1].data_ptr(), vs[1].data_ptr(),
                                           ws.data_ptr(), ws.numel(), st)

        t = timed({"atomic": atomic, "fixed_order": det}, a.reps, a.warmup)
        err = float((vs[0] - vs[1]).abs().max() / vs[1].abs().max())
        row = {"case": label, "B": Bz, "D": Dz, "HW": HWz, "K": Kz, "dtype": str(z.dtype).split(".")[1], "workspace_bytes": ws.numel(),
               "atomic": summary(t["atomic"]), "fixed_order": summary(t["fixed_order"]),
               "ratio_fixed_over_atomic": round(statistics.median(t["fixed_order"]) / statistics.median(t["atomic"]), 3),
               "counts_equal": bool(torch.equal(cs[0], cs[1])), "sums_max_diff_rel_to_max": err}
        row["agree"] = row["counts_equal"] and err <= 1e-5
        rows.append(row)
        print(json.dumps(row), flush=True)

    pats = code_patterns(B, HW, K, dev, g)
    if a.calls_only:
        a.reps, a.warmup = a.calls_only, 0
        stats_case("nchw_f32/uniform", z32, pats["uniform"], B, D, HW, K)
        return
    for name, codes in pats.items():
        stats_case("nchw_f32/" + name, z32, codes, B, D, HW, K)
    zb = z32.to(torch.bfloat16)
    zr = z32.permute(0, 2, 3, 1).reshape(-1, D).contiguous()
    for name, codes in pats.items():
        stats_case("nchw_bf16/" + name, zb, codes, B, D, HW, K)
    for name, codes in pats.items():
        stats_case("rows_f32/" + name, zr, codes, B * HW, D, 1, K)
    del zb, zr
    z4 = torch.randn(B, 4, side, side, device=dev, generator=g)
    stats_case("nchw_f32_D4_K16384/uniform", z4, torch.randint(0, 16384, (B, side, side), device=dev, generator=g), B, 4, HW, 16384)

    # the codebook gradient at the first shape
    E = torch.randn(K, D, device=dev, generator=g)
    gl = torch.tensor([0.5], device=dev)
    gw = [torch.zeros(K, D, device=dev) for _ in range(2)]
    ws = _lib.det_workspace(B, D, HW, K, dev)
    codes, st, coef = pats["uniform"], _lib.stream_ptr(dev), 2.0 / z32.numel()

    def grad_atomic():
        gw[0].zero_()                                                     # the atomic form accumulates: its zero fill is part of its cost
        _lib.checked.dvq_vq_backward_codebook_nchw_f32(z32.data_ptr(), E.data_ptr(), codes.data_ptr(), 0, gl.data_ptr(), coef, B, D, HW, K,
                                                       gw[0].data_ptr(), st)

    def grad_det():
        _lib.checked.dvq_vq_backward_codebook_det_f32(z32.data_ptr(), E.data_ptr(), codes.data_ptr(), 0, gl.data_ptr(), coef, B, D, HW, K,
                                                      gw[1].data_ptr(), ws.data_ptr(), ws.numel(), st)

    t = timed({"atomic": grad_atomic, "fixed_order": grad_det}, a.reps, a.warmup)
    err = float((gw[0] - gw[1]).abs().max() / gw[1].abs().max())
    row = {"case": "codebook_gradient/nchw_f32/uniform", "B": B, "D": D, "HW": HW, "K": K, "workspace_bytes": ws.numel(),
           "atomic": summary(t["atomic"]), "fixed_order": summary(t["fixed_order"]),
           "ratio_fixed_over_atomic": round(statistics.median(t["fixed_order"]) / statistics.median(t["atomic"]), 3),
           "max_diff_rel_to_max": err}
    row["agree"] = err <= 1e-5
    rows.append(row)
    print(json.dumps(row), flush=True)
    del gw, ws

    # a VectorQuantize2 training step: forward, backward, EMA update
    vq = VectorQuantize2(K, D).to(dev).train()
    x = z32.clone().requires_grad_(True)

    def step(flag):
        def run():
            pkg.set_deterministic(flag)
            x.grad = None
            xq, loss, _ = vq(x)
            (xq.sum() + loss).backward()
        return run

    t = timed({"switch_off": step(False), "switch_on": step(True)}, a.reps, a.warmup)
    pkg.set_deterministic(None)
    row = {"case": "VectorQuantize2_training_step", "B": B, "D": D, "HW": HW, "K": K, "switch_off": summary(t["switch_off"]),
           "switch_on": summary(t["switch_on"]),
           "ratio_on_over_off": round(statistics.median(t["switch_on"]) / statistics.median(t["switch_off"]), 3)}
    rows.append(row)
    print(json.dumps(row), flush=True)
    result = {"tool": "tools/det_stats_time.py", "device": torch.cuda.get_device_name(0), "reps": a.reps, "warmup": a.warmup,
              "timing": "HIP events around one call, the two forms alternating, median / min / max of the timed calls", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(a.o)), exist_ok=True)
    with open(a.o, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    bad = [r["case"] for r in rows if not r.get("agree", True)]
    if bad:
        sys.exit("the two forms disagree beyond 1e-5 of the largest entry: %s" % bad)


if __name__ == "__main__":
    main()
