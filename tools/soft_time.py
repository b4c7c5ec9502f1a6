"""get_soft_codes on the fused kernel (`dvq_vq_soft_assign_flat_f32`) against the torch chain it replaced, restated here (the chain
of the commit before the kernel: VQEmbedding.compute_distances' addmm, softmax, argmin / torch.multinomial; for RQBottleneck per
depth, with the hard assign and the residual update around it) -- never against the code under test.  CUDA events, median of
--iters after --warmup, deterministic and stochastic.  Cases:
  vq_n262144   VectorQuantize2, N = 262 144 tokens, K = 1024, D = 256 (BASELINE configs[2])
  rq_n16384    RQBottleneck, N = 16 384, one shared codebook of K = 16 384, D = 256, depth 4 (RQ-VAE's own setting)
  vq_n1024     VectorQuantize2, N = 1024, K = 1024, D = 256 (a single image)
Per case: fused and chain medians, the compute bound 2 N K D (x depth) over the fp32 MFMA peak (157.3 TF/s), and the [N, K] fp32
passes each side makes.  One JSON line per case, the whole record to --out.

    python tools/soft_time.py [--iters 20] [--warmup 3] [--only name] [--out profiles/soft.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd import synth  # noqa: E402
from dynamicvectorquantization_amd.quantize import VectorQuantize2, vq_assign  # noqa: E402
from dynamicvectorquantization_amd.rq import RQBottleneck  # noqa: E402

MFMA_F32_PEAK = 157.3e12
CASES = {
    "vq_n262144": dict(kind="vq", N=262144, K=1024, D=256, temp=32.0),
    "rq_n16384": dict(kind="rq", N=16384, K=16384, D=256, depth=4, temp=64.0),
    "vq_n1024": dict(kind="vq", N=1024, K=1024, D=256, temp=32.0),
}


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


def chain_distances(x, rows):
    norms = (x * x).sum(1, keepdim=True) + (rows * rows).sum(1).unsqueeze(0)
    return torch.addmm(norms, x, rows.t(), alpha=-2.0)


def chain_vq(x, rows, temp, stochastic):
    d = chain_distances(x, rows)
    soft = torch.softmax(d / (-temp), dim=-1)
    code = torch.multinomial(soft, 1).reshape(-1) if stochastic else torch.argmin(d, dim=-1)
    return soft, code


def chain_rq(x, cb, depth, temp, stochastic):
    """per depth: (deterministic) the hard assign kernel for the code, the dense distances and softmax for the soft codes;
    (stochastic) distances, softmax, multinomial; then the residual update"""
    rows = cb.weight[:-1]
    r = x.clone()
    soft, codes = [], []
    for _ in range(depth):
        d = chain_distances(r, rows)
        s = torch.softmax(-d / temp, dim=-1)
        if stochastic:
            c = torch.multinomial(s, 1).reshape(-1)
        else:
            c = vq_assign(r, rows, cb._prep, want_zq=False, want_loss=False)[1]
        r = r - torch.nn.functional.embedding(c, cb.weight)
        soft.append(s.unsqueeze(-2))
        codes.append(c.unsqueeze(-1))
    return torch.cat(soft, dim=-2), torch.cat(codes, dim=-1)


def run_case(name, cfg, iters, warmup):
    dev = torch.device("cuda:0")
    N, K, D, temp = cfg["N"], cfg["K"], cfg["D"], cfg["temp"]
    depth = cfg.get("depth", 1)
    E = torch.from_numpy(synth.codebook_trained(K, D))
    g = torch.Generator().manual_seed(4243)
    pick = torch.randint(0, K, (N,), generator=g)
    x = (E[pick] * (torch.rand(N, 1, generator=g) < 0.5) + 0.6 * torch.randn(N, D, generator=g)).to(dev)
    rec = {"case": name, "N": N, "K": K, "D": D, "depth": depth, "temp": temp,
           "compute_bound_ms": round(2.0 * N * K * D * depth / MFMA_F32_PEAK * 1e3, 4),
           "nk_matrix_bytes": N * K * 4}
    with torch.no_grad():
        if cfg["kind"] == "vq":
            m = VectorQuantize2(K, D, accept_image_fmap=False, channel_last=True).to(dev).eval()
            m.codebook.weight.data[:-1].copy_(E.to(dev))
            m.invalidate_codebook_cache()
            rows = m.codebook.weight[:-1]
            fused = lambda st: m.get_soft_codes(x, temp=temp, stochastic=st)
            chain = lambda st: chain_vq(x, rows, temp, st)
        else:
            m = RQBottleneck((8, 8, D), (8, 8, depth), K, shared_codebook=True).to(dev).eval()
            m.codebooks[0].weight.data[:-1].copy_(E.to(dev))
            m.invalidate_codebook_cache()
            x4 = x.reshape(N // 64, 8, 8, D)
            fused = lambda st: m.get_soft_codes(x4, temp=temp, stochastic=st)
            chain = lambda st: chain_rq(x, m.codebooks[0], depth, temp, st)
        sf, cf = fused(False)
        sc, cc = chain(False)
        rec["hard_codes_match_chain_fraction"] = float((cf.reshape(-1) == cc.reshape(-1)).double().mean())
        rec["soft_max_abs_diff_vs_chain"] = float((sf.reshape(-1, K) - sc.reshape(-1, K)).abs().max())
        del sf, cf, sc, cc
        for st, tag in ((False, "deterministic"), (True, "stochastic")):
            f_ms = median_ms(lambda: fused(st), iters, warmup)
            c_ms = median_ms(lambda: chain(st), iters, warmup)
            rec[tag] = {"fused_ms": round(f_ms, 4), "chain_ms": round(c_ms, 4), "speedup": round(c_ms / f_ms, 2),
                        "fused_over_compute_bound": round(f_ms / rec["compute_bound_ms"], 2)}
    # [N, K] fp32 passes through memory (per depth).  fused: scores written, read back once from HBM / the caches (the second read
    # of a row hits L2), soft written; the draw adds the q write (exponential_) and its read.  chain: addmm writes d; the division
    # reads and writes; softmax reads and writes; argmin reads d -- or multinomial: exponential_ write, a division (two reads, a
    # write), an argmax read.
    rec["nk_passes"] = {"fused_deterministic": 3, "fused_stochastic": 5, "chain_deterministic": 6, "chain_stochastic": 10}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    recs = []
    for name, cfg in CASES.items():
        if a.only and a.only != name:
            continue
        rec = run_case(name, cfg, a.iters, a.warmup)
        print(json.dumps(rec), flush=True)
        recs.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/soft_time.py", "iters": a.iters, "warmup": a.warmup,
                       "fp32_mfma_peak_flops": MFMA_F32_PEAK, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
