"""The narrow-width assign (csrc/vq_assign_narrow.hip) at module level against the reference's op sequence written as torch GPU
ops -- never against the code under test.  HIP events, median of --iters after --warmup.  Cases, each at B = 256 and B = 4 on
32 x 32 latents:
  vqgan_d4_k16384   VectorQuantizer2(16384, 4, beta = 0.25, legacy = False)   (taming-style VQModel checkpoints)
  vq2_d16_k1024     VectorQuantize2(1024, 16)                                  (factorised low-dimensional codebook)
The chain (quantize_vqgan.py:271-312 / quantize2_mask.py:29-55,157-191): NCHW -> NHWC copy, sum of squares of tokens and codes,
addmm for the [N, K] distances, argmin, embedding gather, the two means, z + (z_q - z), NHWC -> NCHW copy.  It is chunked over
tokens where [N, K] fp32 would not fit (--chunk-bytes); at B = 256, K = 16384 the whole matrix would be 17 GB.
Check: our codes equal the chain's on every token whose float64 top-2 distance gap exceeds the fp32 chain's own rounding
(8 ulp of the distance's magnitude); tokens with a float64 gap of exactly zero are ties and counted apart.

    python tools/narrow_time.py --resources-only --out profiles/narrow.json      # no GPU: the kernel resource table (hipcc)
    python tools/narrow_time.py [--iters 20] [--warmup 3] --out profiles/narrow.json    # adds / replaces the timed cases
"""
import argparse
import contextlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {
    "vqgan_d4_k16384": dict(cls="VectorQuantizer2", D=4, K=16384),
    "vq2_d16_k1024": dict(cls="VectorQuantize2", D=16, K=1024),
}
BATCHES = (256, 4)
H = W = 32
BETA = 0.25


def resources():
    """tools/kernel_resources.py's table of vq_assign_narrow.hip as records"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    buf = io.StringIO()
    argv = sys.argv
    sys.argv = ["kernel_resources.py", "vq_assign_narrow.hip"]
    try:
        with contextlib.redirect_stdout(buf):
            kernel_resources.main()
    finally:
        sys.argv = argv
    rows = []
    for ln in buf.getvalue().splitlines():
        name, rest = ln.split(" vgpr ")
        f = rest.split()
        rows.append({"kernel": " ".join(name.split()), "vgpr": int(f[0]), "agpr": int(f[2]), "vgpr_spill": int(f[4]),
                     "scratch_bytes_per_lane": int(f[6]), "lds_bytes_per_block": int(f[8]), "occupancy_waves_per_simd": int(f[10])})
    assert rows and all(r["vgpr_spill"] == 0 and r["scratch_bytes_per_lane"] == 0 for r in rows), "the narrow kernel must not spill"
    return rows


def median_ms(fn, iters, warmup):
    import torch
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


def chain(z, E, chunk_tokens):
    """the reference's forward as torch ops on the GPU -> (z_q NCHW, loss, codes [N])"""
    import torch
    B, D = z.shape[:2]
    rows = z.permute(0, 2, 3, 1).contiguous().reshape(-1, D)
    en = (E * E).sum(1)
    codes = torch.empty(rows.shape[0], dtype=torch.int64, device=z.device)
    for s in range(0, rows.shape[0], chunk_tokens):
        x = rows[s:s + chunk_tokens]
        d = torch.addmm((x * x).sum(1, keepdim=True) + en.unsqueeze(0), x, E.t(), alpha=-2.0)
        codes[s:s + chunk_tokens] = torch.argmin(d, dim=1)
    e = torch.nn.functional.embedding(codes, E)
    m = torch.mean((e - rows) ** 2)
    loss = BETA * m + m
    zq = (rows + (e - rows)).reshape(B, H, W, D).permute(0, 3, 1, 2).contiguous()
    return zq, loss, codes


def check_codes(z, E, ours, theirs, chunk_tokens):
    """tokens by their float64 top-2 gap: ties (gap == 0), near ties (gap within the fp32 chain's rounding), clear"""
    import torch
    D = z.shape[1]
    rows = z.permute(0, 2, 3, 1).reshape(-1, D).double()
    E64 = E.double()
    en = (E64 * E64).sum(1)
    rec = {"tokens": rows.shape[0], "ties": 0, "near_ties": 0, "clear": 0, "clear_mismatches_vs_chain": 0, "clear_mismatches_vs_float64": 0}
    for s in range(0, rows.shape[0], chunk_tokens // 2):
        x = rows[s:s + chunk_tokens // 2]
        xn = (x * x).sum(1, keepdim=True)
        d = torch.addmm(xn + en.unsqueeze(0), x, E64.t(), alpha=-2.0)
        top2, idx = torch.topk(d, 2, dim=1, largest=False)
        gap = top2[:, 1] - top2[:, 0]
        mag = xn.reshape(-1) + en[idx[:, 0]]
        clear = gap > 8.0 * 2.0 ** -23 * mag
        o, t = ours[s:s + x.shape[0]], theirs[s:s + x.shape[0]]
        rec["ties"] += int((gap == 0).sum())
        rec["near_ties"] += int(((gap > 0) & ~clear).sum())
        rec["clear"] += int(clear.sum())
        rec["clear_mismatches_vs_chain"] += int(((o != t) & clear).sum())
        rec["clear_mismatches_vs_float64"] += int(((o != idx[:, 0]) & clear).sum())
    return rec


def run_case(name, cfg, B, iters, warmup, chunk_bytes):
    import torch
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import VectorQuantize2, VectorQuantizer2
    dev = torch.device("cuda:0")
    D, K = cfg["D"], cfg["K"]
    E = synth.codebook_trained(K, D, seed=9501)
    z = torch.from_numpy(synth.z_tokens(E, B, H, W, 9502)).to(dev)
    Et = torch.from_numpy(E).to(dev)
    N = B * H * W
    chunk_tokens = max(1024, min(N, chunk_bytes // (4 * K)))
    with torch.no_grad():
        if cfg["cls"] == "VectorQuantizer2":
            m = VectorQuantizer2(K, D, beta=BETA, legacy=False).to(dev).eval()
            m.embedding.weight.data.copy_(Et)
        else:
            m = VectorQuantize2(K, D, commitment_beta=BETA).to(dev).eval()
            m.codebook.weight.data[:-1].copy_(Et)
        m.invalidate_codebook_cache()
        zq, loss, (_, _, codes) = m(z)
        czq, closs, ccodes = chain(z, Et, chunk_tokens)
        rec = {"case": name, "B": B, "N": N, "K": K, "D": D, "nk_matrix_bytes": N * K * 4, "chain_chunk_tokens": chunk_tokens,
               "codes": check_codes(z, Et, codes.reshape(-1), ccodes, chunk_tokens),
               "loss": float(loss), "chain_loss": float(closs)}
        del czq, ccodes
        ours = median_ms(lambda: m(z), iters, warmup)
        theirs = median_ms(lambda: chain(z, Et, chunk_tokens), iters, warmup)
    rec.update(module_forward_ms=round(ours, 4), torch_chain_ms=round(theirs, 4), speedup=round(theirs / ours, 2),
               lane_ops=N * K * (D + 4))
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--chunk-bytes", type=int, default=2 << 30)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    doc = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            doc = json.load(f)
    doc["tool"] = "tools/narrow_time.py"
    if a.resources_only:
        doc["kernel_resources"] = resources()
        doc.setdefault("cases", "not timed")
        print(json.dumps(doc["kernel_resources"], indent=1))
    else:
        import torch
        recs = []
        for name, cfg in CASES.items():
            for B in BATCHES:
                rec = run_case(name, cfg, B, a.iters, a.warmup, a.chunk_bytes)
                print(json.dumps(rec), flush=True)
                recs.append(rec)
        doc.update(iters=a.iters, warmup=a.warmup, device=torch.cuda.get_device_name(0), cases=recs)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
    if not a.resources_only:
        bad = [r["case"] for r in doc["cases"] if r["codes"]["clear_mismatches_vs_chain"] or r["codes"]["clear_mismatches_vs_float64"]]
        if bad:
            sys.exit("codes differ from the torch chain on clearly decided tokens: %s" % bad)


if __name__ == "__main__":
    main()
