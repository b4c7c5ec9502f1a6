"""The lucidrains-style VectorQuantize (dynamicvectorquantization_amd/lucid.py) on the HIP kernels against the torch-op restatement
of the reference's op sequence (kept here: quantize_lucidrains.py:108-149 and :344-391 with common_utils, op for op, on the same
GPU) -- never against the code under test.  HIP events, median of --iters after --warmup, one process.  Cases:
  step_temp0 / step_temp1   one training step (forward, the codebook update, backward to x) of VectorQuantize, B = 256, 32 x 32,
                            D = 256, K = 1024 (N = 262 144 tokens), decay 0.8, no expiry; sample_codebook_temp 0 and 1.0
  ortho_n1024 / ortho_n16384   orthogonal_loss_fn forward + backward, D = 256
One JSON line per case, the whole record to --out.

    python tools/lucid_prof.py [--iters 10] [--warmup 2] [--batch 256] [--out profiles/lucid.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd import lucid, synth  # noqa: E402

MFMA_F32_PEAK = 157.3e12


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


def log_(t, eps=1e-20):
    return torch.log(t.clamp(min=eps))


def chain_step(x, state, decay, eps, temp, cw):
    """the reference's training-mode forward (accept_image_fmap=True, Euclidean codebook, threshold_ema_dead_code = 0) and the
    backward to x, in its own torch ops; `state` = dict(embed [1, K, D], embed_avg, cluster_size [1, K])"""
    x = x.detach().requires_grad_(True)
    b, c, height, width = x.shape
    K = state["embed"].shape[1]
    xr = x.permute(0, 2, 3, 1).reshape(b, height * width, c)
    xc = xr.float().unsqueeze(0)                                            # '... -> 1 ...'
    flatten = xc.reshape(1, -1, c)
    embed = state["embed"]
    dist = -torch.cdist(flatten, embed, p=2)
    if temp == 0:
        ind = dist.argmax(dim=-1)
    else:
        ind = ((dist / temp) + (-log_(-log_(torch.zeros_like(dist).uniform_(0, 1))))).argmax(dim=-1)
    onehot = F.one_hot(ind, K).type(flatten.dtype)
    ind = ind.view(1, b, height * width)
    quantize = embed.unsqueeze(1).expand(1, b, K, c).gather(2, ind.unsqueeze(-1).expand(1, b, height * width, c))
    with torch.no_grad():
        cluster_size = onehot.sum(dim=1)
        state["cluster_size"].mul_(decay).add_(cluster_size, alpha=(1 - decay))
        embed_sum = torch.einsum('h n d, h n c -> h c d', flatten, onehot)  # (computed and dropped, as the reference does)
        cs = (state["cluster_size"] + eps) / (state["cluster_size"].sum() + K * eps) * state["cluster_size"].sum()
        state["embed"].copy_(state["embed_avg"] / cs.unsqueeze(-1))
        del embed_sum
    quantize, ind = quantize[0], ind[0]
    quantize = xr + (quantize - xr).detach()
    loss = torch.tensor([0.], device=x.device, requires_grad=True)
    loss = loss + F.mse_loss(quantize.detach(), xr) * cw
    quantize = quantize.reshape(b, height, width, c).permute(0, 3, 1, 2)
    (loss.sum() + quantize.sum()).backward()
    return quantize, loss, ind.reshape(b, height, width), x.grad


def chain_ortho(t):
    t = t.detach().requires_grad_(True)
    h, n = t.shape[:2]
    normed = F.normalize(t, p=2, dim=-1)
    identity = torch.eye(n, device=t.device).unsqueeze(0).expand(h, n, n)
    cosine_sim = torch.einsum('h i d, h j d -> h i j', normed, normed)
    loss = ((cosine_sim - identity) ** 2).sum() / (h * n ** 2)
    loss.backward()
    return loss, t.grad


def fused_ortho(t):
    t = t.detach().requires_grad_(True)
    loss = lucid.orthogonal_loss_fn(t)
    loss.backward()
    return loss, t.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, D, H, W, K = a.batch, 256, 32, 32, 1024
    N = B * H * W
    E = torch.from_numpy(synth.codebook_trained(K, D)).to(dev)
    g = torch.Generator().manual_seed(4246)
    pick = torch.randint(0, K, (N,), generator=g)
    rows = E.cpu()[pick] * (torch.rand(N, 1, generator=g) < 0.5) + 0.6 * torch.randn(N, D, generator=g)
    x = rows.reshape(B, H * W, D).permute(0, 2, 1).reshape(B, D, H, W).contiguous().to(dev)
    del rows
    recs = []
    for name, temp in (("step_temp0", 0.0), ("step_temp1", 1.0)):
        m = lucid.VectorQuantize(K, D, decay=0.8, accept_image_fmap=True, sample_codebook_temp=temp).to(dev).train()
        with torch.no_grad():
            m._codebook.embed.copy_(E.unsqueeze(0))
            m._codebook.embed_avg.copy_(E.unsqueeze(0))
            m._codebook.cluster_size.fill_(float(N) / K)
        state = dict(embed=E.unsqueeze(0).clone(), embed_avg=E.unsqueeze(0).clone(),
                     cluster_size=torch.full((1, K), float(N) / K, device=dev))

        def fused():
            xin = x.detach().requires_grad_(True)
            q, loss, (_, _, ind) = m(xin)
            (loss.sum() + q.sum()).backward()
            return q, loss, ind, xin.grad

        chain = lambda: chain_step(x, state, 0.8, 1e-5, temp, 1.0)
        rec = {"case": name, "B": B, "D": D, "H": H, "W": W, "K": K, "N": N, "temp": temp,
               "compute_bound_ms": round(2.0 * N * K * D / MFMA_F32_PEAK * 1e3, 4)}
        if temp == 0:
            _, loss_f, ind_f, gx_f = fused()
            _, loss_c, ind_c, gx_c = chain()
            rec["codes_match_chain_fraction"] = float((ind_f == ind_c).double().mean())
            rec["loss_rel_diff_vs_chain"] = abs(float(loss_f.detach()) - float(loss_c.detach())) / abs(float(loss_c.detach()))
            del ind_f, ind_c, gx_f, gx_c
        f_ms = median_ms(fused, a.iters, a.warmup)
        c_ms = median_ms(chain, a.iters, a.warmup)
        rec.update(fused_ms=round(f_ms, 4), chain_ms=round(c_ms, 4), speedup=round(c_ms / f_ms, 2))
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        del m, state
        torch.cuda.empty_cache()
    for n in (1024, 16384):
        t = torch.from_numpy(synth.codebook_trained(n, D, seed=4247)).to(dev).unsqueeze(0)
        lf, gf = fused_ortho(t)
        lc, gc = chain_ortho(t)
        rec = {"case": "ortho_n%d" % n, "n": n, "D": D,
               "loss_rel_diff_vs_chain": abs(float(lf.detach()) - float(lc.detach())) / abs(float(lc.detach())),
               "grad_max_abs_diff_vs_chain_over_max": float((gf - gc).abs().max() / gc.abs().max()),
               "forward_flop": 2.0 * n * n * D / 2, "backward_flop": 2.0 * 2.0 * n * n * D,
               "nxn_bytes": n * n * 4}
        del gf, gc
        f_ms = median_ms(lambda: fused_ortho(t), a.iters, a.warmup)
        c_ms = median_ms(lambda: chain_ortho(t), a.iters, a.warmup)
        ff_ms = median_ms(lambda: lucid.orthogonal_loss_fn(t), a.iters, a.warmup)
        rec.update(fused_ms=round(f_ms, 4), chain_ms=round(c_ms, 4), speedup=round(c_ms / f_ms, 2), fused_forward_ms=round(ff_ms, 4),
                   compute_bound_ms=round((rec["forward_flop"] + rec["backward_flop"]) / MFMA_F32_PEAK * 1e3, 4))
        print(json.dumps(rec), flush=True)
        recs.append(rec)
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/lucid_prof.py", "iters": a.iters, "warmup": a.warmup,
                       "fp32_mfma_peak_flops": MFMA_F32_PEAK, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
