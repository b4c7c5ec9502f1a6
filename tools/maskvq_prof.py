"""MaskVectorQuantize's forward on the HIP kernels against the torch-op restatement of the reference's forward (kept here:
quantize_codebook_mask.py:77-144 with common_utils.gumbel_sample, op for op) on the same GPU -- never against the code under
test.  torch.no_grad(), HIP events, median of --iters after --warmup, one process.  Shape: B = 256, D = 256, 32 x 32, K = 1024
(N = 262 144 tokens; `u` is 1 GiB).  Cases:
  l2_temp0     L2, temp = 0: `vq_assign` (the filter path); beside it VectorQuantize2's forward at the same shape -- the same op,
               the two must cost the same up to the mask ratio's multiply
  l2_temp1     L2, temp = 1: the N x K draw, `dvq_vq_score_assign_f32`, `dvq_vq_apply_codes_nchw_f32`; also without the draw
  cos_temp1    use_cosine_sim, temp = 1: the NHWC copy and two F.normalize, then the same two kernels
One JSON line per case, the whole record to --out.

    python tools/maskvq_prof.py [--iters 20] [--warmup 3] [--batch 256] [--out profiles/maskvq.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd import synth  # noqa: E402
from dynamicvectorquantization_amd.quantize import MaskVectorQuantize, VectorQuantize2  # noqa: E402

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


def chain_forward(x, weight, beta, temp, mask, cosine):
    """the reference's forward in its own torch ops (accept_image_fmap=True)"""
    height, width = x.shape[-2:]
    b, c = x.shape[:2]
    x = x.permute(0, 2, 3, 1).reshape(b, height * width, c).contiguous()
    if mask is not None:
        mask = mask.permute(0, 2, 3, 1).reshape(b, height * width, 1).contiguous()
    shape = x.shape
    flatten = x
    if cosine:
        fn = F.normalize(flatten, p=2, dim=-1)
        wn = F.normalize(weight, p=2, dim=-1).unsqueeze(0)
        dist = torch.einsum('hnd,hcd->hnc', fn, wn)
    else:
        flatten = flatten.view(-1, c)
        dist = - torch.sum(flatten ** 2, dim=1, keepdim=True) - torch.sum(weight ** 2, dim=1) + 2 * \
            torch.einsum('bd,dn->bn', flatten, weight.t())
    if temp == 0:
        ind = dist.argmax(dim=-1)
    else:
        noise = torch.zeros_like(dist).uniform_(0, 1)
        ind = ((dist / temp) + (-log_(-log_(noise)))).argmax(dim=-1)
    ind = ind.view(*shape[:-1])
    x_q = F.embedding(ind, weight)
    if mask is not None:
        ratio = 1 / torch.mean(mask)
        loss = ratio * beta * torch.mean((x_q - x) ** 2 * mask) + ratio * torch.mean((x_q - x) ** 2 * mask)
    else:
        loss = beta * torch.mean((x_q - x) ** 2) + torch.mean((x_q - x) ** 2)
    x_q = x + (x_q - x)
    x_q = x_q.reshape(b, height, width, c).permute(0, 3, 1, 2).contiguous()
    return x_q, loss, ind.reshape(b, height, width)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    B, D, H, W, K = a.batch, 256, 32, 32, 1024
    N = B * H * W
    E = torch.from_numpy(synth.codebook_trained(K, D)).to(dev)
    g = torch.Generator().manual_seed(4245)
    pick = torch.randint(0, K, (N,), generator=g)
    rows = E.cpu()[pick] * (torch.rand(N, 1, generator=g) < 0.5) + 0.6 * torch.randn(N, D, generator=g)
    x = rows.reshape(B, H * W, D).permute(0, 2, 1).reshape(B, D, H, W).contiguous().to(dev)
    del rows
    mask = (torch.rand(B, 1, H, W, generator=g) < 0.6).float().to(dev)
    recs = []
    base = {"B": B, "D": D, "H": H, "W": W, "K": K, "N": N, "u_bytes": N * K * 4, "z_bytes": N * D * 4,
            "compute_bound_ms": round(2.0 * N * K * D / MFMA_F32_PEAK * 1e3, 4)}
    with torch.no_grad():
        vq2 = VectorQuantize2(K, D).to(dev).eval()
        vq2.codebook.weight.data[:-1].copy_(E)
        vq2.invalidate_codebook_cache()
        for name, cosine, temp in (("l2_temp0", False, 0.0), ("l2_temp1", False, 1.0), ("cos_temp1", True, 1.0)):
            m = MaskVectorQuantize(K, D, use_cosine_sim=cosine).to(dev).eval()
            m.embedding.weight.data.copy_(E)
            m.invalidate_codebook_cache()
            w = m.embedding.weight.detach()
            fused = lambda: m(x, temp=temp, codebook_mask=mask)
            chain = lambda: chain_forward(x, w, float(m.beta), temp, mask, cosine)
            rec = dict(base, case=name, cosine=cosine, temp=temp)
            xq_f, loss_f, (_, _, ind_f) = fused()
            if temp == 0:
                xq_c, loss_c, ind_c = chain()
                rec["codes_match_chain_fraction"] = float((ind_f == ind_c).double().mean())
                rec["loss_rel_diff_vs_chain"] = abs(float(loss_f) - float(loss_c)) / abs(float(loss_c))
                del xq_c, ind_c
            del xq_f, ind_f
            f_ms = median_ms(fused, a.iters, a.warmup)
            c_ms = median_ms(chain, a.iters, a.warmup)
            rec.update(fused_ms=round(f_ms, 4), chain_ms=round(c_ms, 4), speedup=round(c_ms / f_ms, 2),
                       fused_over_compute_bound=round(f_ms / base["compute_bound_ms"], 2))
            if temp == 0:
                v_ms = median_ms(lambda: vq2(x, codebook_mask=mask), a.iters, a.warmup)
                rec.update(vector_quantize2_ms=round(v_ms, 4), over_vector_quantize2=round(f_ms / v_ms, 3))
            else:
                u = torch.zeros(N, K, device=dev).uniform_(0, 1)
                m._draw_uniform = lambda N_, K_, device: u          # the same forward without the draw: what the kernels cost
                rec["fused_without_draw_ms"] = round(median_ms(fused, a.iters, a.warmup), 4)
                rec["draw_ms"] = round(median_ms(lambda: torch.zeros(N, K, device=dev).uniform_(0, 1), a.iters, a.warmup), 4)
                del u
            print(json.dumps(rec), flush=True)
            recs.append(rec)
            del m
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"tool": "tools/maskvq_prof.py", "iters": a.iters, "warmup": a.warmup,
                       "fp32_mfma_peak_flops": MFMA_F32_PEAK, "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
