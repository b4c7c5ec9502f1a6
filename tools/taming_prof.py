"""VectorQuantizer / EMAVectorQuantizer (the fused assign + `dvq_code_stats_f32`, the EMA kernels) against the torch-op chain of the
reference's forwards, restated here op for op (quantize_vqgan.py:34-90 and :419-457) on the same GPU -- never against the code
under test.  torch.no_grad() forwards, HIP events, median of --iters after --warmup, the two sides alternated --rounds times in
one process (both medians of every round are kept).  Shapes: B = 256, 32 x 32 with (K, D) = (1024, 256) and (16384, 4); the
one-hot matrix is N x K x 4 bytes = 1 GiB / 16 GiB, so is the chain's distance matrix.  Also timed: `code_usage` alone with the
one-hot write, against its bound N K 4 bytes over the HBM write bandwidth.  One JSON line, the whole record to --out.

    python tools/taming_prof.py [--iters 10] [--warmup 3] [--rounds 2] [--batch 256] [--out profiles/taming.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd.quantize import EMAVectorQuantizer, VectorQuantizer, code_usage  # noqa: E402

HBM_PEAK = 8.0e12                       # bytes / s, MI355X data sheet


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


def chain_vq(z, weight, beta):
    """VectorQuantizer.forward in the reference's own torch ops"""
    n_e, e_dim = weight.shape
    z = z.permute(0, 2, 3, 1).contiguous()
    zf = z.view(-1, e_dim)
    d = torch.sum(zf ** 2, dim=1, keepdim=True) + torch.sum(weight ** 2, dim=1) - 2 * torch.matmul(zf, weight.t())
    idx = torch.argmin(d, dim=1).unsqueeze(1)
    enc = torch.zeros(idx.shape[0], n_e).to(z)
    enc.scatter_(1, idx, 1)
    z_q = torch.matmul(enc, weight).view(z.shape)
    loss = torch.mean((z_q.detach() - z) ** 2) + beta * torch.mean((z_q - z.detach()) ** 2)
    z_q = z + (z_q - z).detach()
    e_mean = torch.mean(enc, dim=0)
    perplexity = torch.exp(-torch.sum(e_mean * torch.log(e_mean + 1e-10)))
    return z_q.permute(0, 3, 1, 2).contiguous(), loss, (perplexity, enc, idx)


def chain_ema(z, emb, beta, train):
    """EMAVectorQuantizer.forward in the reference's own torch ops; emb: dict(weight, cluster_size, embed_avg, decay, eps)"""
    w = emb["weight"]
    K, D = w.shape
    z = z.permute(0, 2, 3, 1)
    zf = z.reshape(-1, D)
    d = zf.pow(2).sum(dim=1, keepdim=True) + w.pow(2).sum(dim=1) - 2 * torch.einsum('bd,nd->bn', zf, w)
    idx = torch.argmin(d, dim=1)
    z_q = F.embedding(idx, w).view(z.shape)
    enc = F.one_hot(idx, K).type(z.dtype)
    avg_probs = torch.mean(enc, dim=0)
    perplexity = torch.exp(-torch.sum(avg_probs * torch.log(avg_probs + 1e-10)))
    if train:
        emb["cluster_size"].mul_(emb["decay"]).add_(enc.sum(0), alpha=1 - emb["decay"])
        emb["embed_avg"].mul_(emb["decay"]).add_(enc.transpose(0, 1) @ zf, alpha=1 - emb["decay"])
        n = emb["cluster_size"].sum()
        smoothed = (emb["cluster_size"] + emb["eps"]) / (n + K * emb["eps"]) * n
        w.copy_(emb["embed_avg"] / smoothed.unsqueeze(1))
    loss = beta * F.mse_loss(z_q.detach(), z)
    z_q = z + (z_q - z).detach()
    return z_q.permute(0, 3, 1, 2), loss, (perplexity, enc, idx)


def run_shape(B, K, D, a, dev):
    H = W = 32
    N = B * H * W
    torch.manual_seed(4400 + D)
    E = torch.randn(K, D, device=dev) * 0.5
    z = torch.randn(B, D, H, W, device=dev)
    j = torch.randint(0, K, (N,), device=dev)
    z = torch.where(torch.rand(B, 1, H, W, device=dev) < 0.5, E[j].view(B, H, W, D).permute(0, 3, 1, 2) + 0.3 * z, z).contiguous()
    rec = {"B": B, "H": H, "W": W, "K": K, "D": D, "N": N, "onehot_bytes": N * K * 4,
           "onehot_write_bound_ms": round(N * K * 4 / HBM_PEAK * 1e3, 4)}
    vq = VectorQuantizer(K, D, 0.25).to(dev).eval()
    ema = EMAVectorQuantizer(K, D, 0.25).to(dev)
    emb = dict(weight=E.clone(), cluster_size=torch.ones(K, device=dev), embed_avg=E.clone(), decay=0.99, eps=1e-5)
    with torch.no_grad():
        vq.embedding.weight.copy_(E)
        ema.embedding.weight.copy_(E)
        ema.embedding.embed_avg.copy_(E)
        ema.embedding.cluster_size.fill_(1.0)
        # the two sides agree before anything is timed (fp32 distances by a vendor GEMM: near-ties may differ)
        zq_f, loss_f, (p_f, enc_f, idx_f) = vq(z)
        zq_c, loss_c, (p_c, enc_c, idx_c) = chain_vq(z, E, 0.25)
        same = idx_f.reshape(-1) == idx_c.reshape(-1)
        rec["codes_match_chain_fraction"] = float(same.double().mean())
        rec["perplexity"] = float(p_f)
        rec["perplexity_rel_diff_vs_chain"] = abs(float(p_f) - float(p_c)) / float(p_c)
        rec["loss_rel_diff_vs_chain"] = abs(float(loss_f) - float(loss_c)) / abs(float(loss_c))
        rec["onehot_equal_where_codes_match"] = bool(torch.equal(enc_f[same], enc_c[same]))
        del zq_f, zq_c, enc_f, enc_c, same
        torch.cuda.empty_cache()
        codes = idx_f.reshape(-1).contiguous()
        sides = {
            "vq_ms": lambda: vq(z), "vq_chain_ms": lambda: chain_vq(z, E, 0.25),
            "ema_eval_ms": lambda: ema.eval()(z), "ema_eval_chain_ms": lambda: chain_ema(z, emb, 0.25, False),
            "ema_train_ms": lambda: ema.train()(z), "ema_train_chain_ms": lambda: chain_ema(z, emb, 0.25, True),
            "code_usage_onehot_ms": lambda: code_usage(codes, K, want_encodings=True),
            "code_usage_ms": lambda: code_usage(codes, K),
        }
        for name in sides:
            rec[name] = []
        for _ in range(a.rounds):
            for name, fn in sides.items():
                rec[name].append(round(median_ms(fn, a.iters, a.warmup), 4))
                torch.cuda.empty_cache()
        vq.want_encodings = False
        rec["vq_without_encodings_ms"] = round(median_ms(lambda: vq(z), a.iters, a.warmup), 4)
    best = lambda k: min(rec[k])
    rec["onehot_write_GBps"] = round(N * K * 4 / (best("code_usage_onehot_ms") * 1e-3) / 1e9, 1)
    rec["chain_over_ours"] = {k: round(best(k + "_chain_ms") / best(k + "_ms"), 2) for k in ("vq", "ema_eval", "ema_train")}
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/taming_prof.py measures on the GPU: none found")
    dev = torch.device("cuda:0")
    rec = {"tool": "tools/taming_prof.py", "iters": a.iters, "warmup": a.warmup, "rounds": a.rounds,
           "timing": "HIP events around one forward, median per round; chain = the reference's torch ops on the same GPU",
           "shapes": [run_shape(a.batch, K, D, a, dev) for K, D in ((1024, 256), (16384, 4))]}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
