"""GumbelQuantize's fused forward (`dvq_vq_gumbel_assign_f32`) against the torch-op chain of the reference's forward, restated here
(quantize_vqgan.py:171-200, op for op) on the same GPU -- never against the code under test.  torch.no_grad(), eval mode, HIP
events, median of --iters after --warmup, one process.  Shape: B = 256, C = 256, 32 x 32, K = 1024, d = 256 (N = 262 144 tokens;
the logits, and the variates q, are 1 GiB each).  Timed: the module's forward (draw included), the same with the variates given
(what the kernel sweep costs), the draw alone, the chain (its own draw included).  Also written: the near-tie margin of the
tests' fixture.  One JSON line, the whole record to --out.

    python tools/gumbel_prof.py [--iters 20] [--warmup 5] [--batch 256] [--out profiles/gumbel.json]

--train: the training leg instead -- forward + backward of the SAME module in training mode with `fused_backward` off (the torch-op
chain under autograd) and on (the sweep that keeps the logits, the streaming backward kernel, vendor GEMMs), in the same run: HIP
events, median of --iters after --warmup, and torch.cuda.max_memory_allocated of each, at B = 256, C = 256, 32 x 32, K = 1024,
d = 256 and at B = 16, C = 256, 32 x 32, K = 8192, d = 256.  The loss is sum(z_q G) + diff with a fixed G ~ N(0, 1); the draw of the
variates is inside both.

    python tools/gumbel_prof.py --train [--iters 20] [--warmup 5] [--out profiles/gumbel_train.json]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd.quantize import GumbelQuantize  # noqa: E402

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


def chain_forward(z, proj, embed, n_embed, kl_weight, temp):
    """the reference's forward in its own torch ops (eval: hard = True, no remap)"""
    logits = proj(z)
    soft_one_hot = F.gumbel_softmax(logits, tau=temp, dim=1, hard=True)
    z_q = torch.einsum('b n h w, n d -> b d h w', soft_one_hot, embed.weight)
    qy = F.softmax(logits, dim=1)
    diff = kl_weight * torch.sum(qy * torch.log(qy * n_embed + 1e-10), dim=1).mean()
    ind = soft_one_hot.argmax(dim=1)
    return z_q, diff, ind


TRAIN_SHAPES = ((256, 256, 32, 32, 1024, 256), (16, 256, 32, 32, 8192, 256))     # B, C, H, W, K, d


def train_leg(dev, iters, warmup):
    rec = {"tool": "tools/gumbel_prof.py --train", "iters": iters, "warmup": warmup, "shapes": []}
    for B, C, H, W, K, d in TRAIN_SHAPES:
        torch.manual_seed(4302)
        m = GumbelQuantize(C, d, K).to(dev).train()
        with torch.no_grad():
            m.proj.weight.normal_(0.0, 1.5 / C ** 0.5)
            m.proj.bias.normal_(0.0, 0.5)
        z = torch.randn(B, C, H, W, device=dev, requires_grad=True)
        G = torch.randn(B, d, H, W, device=dev)
        one = torch.ones((), device=dev)

        def step():
            z.grad = None
            for p in m.parameters():
                p.grad = None
            z_q, diff, _ = m(z)
            torch.autograd.backward([z_q, diff], [G, one])

        row = {"B": B, "C": C, "H": H, "W": W, "K": K, "d": d, "N": B * H * W, "logits_bytes": B * H * W * K * 4}
        for name, flag in (("torch", False), ("fused", True)):
            m.fused_backward = flag
            torch.cuda.empty_cache()
            torch.cuda.reset_peak_memory_stats(dev)
            ms = median_ms(step, iters, warmup)
            assert m.last_path == ("fused_train" if flag else "torch"), m.last_path
            row[name + "_ms"] = round(ms, 4)
            row[name + "_max_memory_allocated"] = int(torch.cuda.max_memory_allocated(dev))
        row["speedup"] = round(row["torch_ms"] / row["fused_ms"], 2)
        rec["shapes"].append(row)
        del m, z, G
        torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--train", action="store_true")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    if a.train:
        rec = train_leg(dev, a.iters, a.warmup)
        print(json.dumps(rec), flush=True)
        if a.out:
            with open(a.out, "w") as f:
                json.dump(rec, f, indent=1)
        return
    B, C, H, W, K, d = a.batch, 256, 32, 32, 1024, 256
    N = B * H * W
    torch.manual_seed(4301)
    m = GumbelQuantize(C, d, K).to(dev).eval()
    with torch.no_grad():
        m.proj.weight.normal_(0.0, 1.5 / C ** 0.5)
        m.proj.bias.normal_(0.0, 0.5)
    z = torch.randn(B, C, H, W, device=dev)
    rec = {"tool": "tools/gumbel_prof.py", "iters": a.iters, "warmup": a.warmup, "B": B, "C": C, "H": H, "W": W, "K": K, "d": d,
           "N": N, "q_bytes": N * K * 4, "z_bytes": N * C * 4, "zq_bytes": N * d * 4,
           "compute_bound_ms": round(2.0 * N * K * C / MFMA_F32_PEAK * 1e3, 4)}
    try:
        from tests import _gumbel_ref as R
        meta = R.load()["meta"]
        rec.update(near_tie_margin=meta["margin"], err_ref=meta["err_ref"], margin_factor=meta["factor"])
    except Exception as e:                                       # the fixture is test data: the timing does not need it
        rec["near_tie_margin"] = "unavailable: %s" % e
    with torch.no_grad():
        q = torch.empty(B, K, H, W, device=dev).exponential_()
        zq_f, diff_f, (_, _, ind_f) = m(z, q=q)
        # the chain with the same variates: torch's own ops on the same logits
        logits = m.proj(z)
        ind_c = ((logits - q.log()) / m.temperature).argmax(1)
        qy = F.softmax(logits, dim=1)
        diff_c = m.kl_weight * torch.sum(qy * torch.log(qy * K + 1e-10), dim=1).mean()
        rec["codes_match_chain_fraction"] = float((ind_f == ind_c).double().mean())
        rec["diff_rel_diff_vs_chain"] = abs(float(diff_f) - float(diff_c)) / abs(float(diff_c))
        rec["zq_is_codebook_row"] = bool(torch.equal(zq_f, m.embed.weight[ind_f].permute(0, 3, 1, 2)))
        del logits, ind_c, qy, zq_f, ind_f
        torch.cuda.empty_cache()
        fused = lambda: m(z)
        f_ms = median_ms(fused, a.iters, a.warmup)
        k_ms = median_ms(lambda: m(z, q=q), a.iters, a.warmup)
        d_ms = median_ms(lambda: torch.empty(B, K, H, W, device=dev).exponential_(), a.iters, a.warmup)
        del q
        torch.cuda.empty_cache()
        c_ms = median_ms(lambda: chain_forward(z, m.proj, m.embed, K, m.kl_weight, m.temperature), a.iters, a.warmup)
    rec.update(fused_ms=round(f_ms, 4), fused_without_draw_ms=round(k_ms, 4), draw_ms=round(d_ms, 4), chain_ms=round(c_ms, 4),
               speedup=round(c_ms / f_ms, 2), fused_without_draw_over_compute_bound=round(k_ms / rec["compute_bound_ms"], 2))
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
