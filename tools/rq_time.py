"""Residual quantization (RQBottleneck on the HIP assign path) against a torch-op restatement of the reference's sequence
(quantize_rqvae.py:237-296: per depth addmm distances / argmin / embedding / sub_ / add_, the commitment loss, the straight-through
output).  CUDA events, median of --iters after --warmup.  Cases:
  get_codes_b256   eval forward, B = 256, latent (8, 8, 256), shared K = 16384, depth 4 (RQ-VAE's own setting, N = 16384)
  get_codes_b32    the same at B = 32
  rqvae_default    RQVAE's defaults: embed_dim 64, K = 512, latent (8, 8, 64), code (8, 8, 4), B = 256
  train_b64        training forward + backward (loss sum(out * R) + loss), shared K = 16384, D = 256, depth 4, B = 64
Per case: the op's median, the torch ops' median, and for the eval cases a per-depth split (events between the assign and the step
kernel of each depth, run as the module runs them) with the step kernel's achieved HBM fraction (its tensor streams over 6.29 TB/s,
the measured float4-copy ceiling) and the assign's TF/s (2 N K D flops of the distance product).  One JSON line per case, and the
whole record to --out.

    python tools/rq_time.py [--iters 30] [--warmup 5] [--only name] [--out profiles/rq.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd import _lib, synth  # noqa: E402
from dynamicvectorquantization_amd.quantize import vq_assign  # noqa: E402
from dynamicvectorquantization_amd.rq import RQBottleneck  # noqa: E402

HBM = 6.29e12
CASES = {
    "get_codes_b256": dict(latent=(8, 8, 256), code=(8, 8, 4), K=16384, B=256, train=False),
    "get_codes_b32": dict(latent=(8, 8, 256), code=(8, 8, 4), K=16384, B=32, train=False),
    "rqvae_default": dict(latent=(8, 8, 64), code=(8, 8, 4), K=512, B=256, train=False),
    "train_b64": dict(latent=(8, 8, 256), code=(8, 8, 4), K=16384, B=64, train=True),
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


def torch_ops(x, W, depth, train_grad=False):
    """the reference's eval sequence with one shared codebook W [K + 1, D] as torch ops (rH = rW = 1)"""
    B, H, Wd, D = x.shape
    E = W[:-1]
    en = E.pow(2.0).sum(dim=1).unsqueeze(0)
    xf = x.reshape(-1, D)
    r = xf.detach().clone()
    agg = torch.zeros_like(xf)
    losses = []
    codes = []
    for _ in range(depth):
        d = torch.addmm(r.pow(2.0).sum(dim=1, keepdim=True) + en, r, E.t(), alpha=-2.0)
        c = d.argmin(dim=-1)
        q = torch.nn.functional.embedding(c, W)
        r.sub_(q)
        agg.add_(q)
        losses.append((xf - agg.detach()).pow(2.0).mean())
        codes.append(c)
    loss = torch.mean(torch.stack(losses))
    out = x + (agg.reshape(x.shape) - x).detach()
    return out, loss, torch.stack(codes, -1)


def split(rq, x, iters, warmup):
    """per-depth (assign ms, step ms) of the eval forward, the module's own calls with events in between"""
    L = _lib.lib
    B, H, W, Dl = x.shape
    depth, D, N = rq.code_shape[-1], Dl, B * H * W
    cb = rq.codebooks[0]
    ws = torch.empty(L.dvq_rq_workspace_bytes(N, D, depth, 0), dtype=torch.uint8, device=x.device)
    codes = torch.empty((B, H, W, depth), dtype=torch.int64, device=x.device)
    out = torch.empty_like(x)
    c = torch.empty(N, dtype=torch.int64, device=x.device)
    st = _lib.stream_ptr(x.device)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * depth + 1)]

    def run(record):
        r = x.view(N, D)
        if record:
            ev[0].record()
        for i in range(depth):
            vq_assign(r, cb.weight[:-1], cb._prep, want_zq=False, want_loss=False, mode=rq.assign_mode, out=(None, c, None))
            if record:
                ev[2 * i + 1].record()
            _lib.check(L.dvq_rq_step_f32(x.data_ptr(), r.data_ptr(), cb.weight.data_ptr(), cb.n_embed, c.data_ptr(), B, H, W, 1, 1,
                                         Dl, D, i, depth, 0, codes.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), st), "step")
            if record:
                ev[2 * i + 2].record()
            if i + 1 < depth:
                off = L.dvq_rq_residual_offset(N, D, depth, i + 1)
                r = ws[off:off + N * D * 4].view(torch.float32).view(N, D)

    for _ in range(warmup):
        run(False)
    samples = []
    for _ in range(iters):
        run(True)
        ev[-1].synchronize()
        samples.append([ev[k].elapsed_time(ev[k + 1]) for k in range(2 * depth)])
    med = [sorted(s[k] for s in samples)[len(samples) // 2] for k in range(2 * depth)]
    K = cb.n_embed
    rows = []
    for i in range(depth):
        a_ms, s_ms = med[2 * i], med[2 * i + 1]
        # step streams: read x, r_i (and agg_i for i > 0), write r_{i+1} and agg_{i+1} (last depth: out only), + codes
        nbytes = N * D * 4 * (2 + (i > 0) + (1 if i == depth - 1 else 2)) + N * 16
        rows.append({"depth": i, "assign_us": round(a_ms * 1e3, 1), "step_us": round(s_ms * 1e3, 1),
                     "assign_tflops": round(2.0 * N * K * D / (a_ms * 1e-3) / 1e12, 1),
                     "step_bytes": nbytes, "step_hbm_fraction": round(nbytes / (s_ms * 1e-3) / HBM, 3)})
    return rows


def run_case(name, cfg, iters, warmup):
    dev = torch.device("cuda:0")
    rq = RQBottleneck(cfg["latent"], cfg["code"], cfg["K"], shared_codebook=True)
    Dl = cfg["latent"][2]
    with torch.no_grad():
        rq.codebooks[0].weight[:-1].copy_(torch.from_numpy(synth.codebook_trained(cfg["K"], Dl)))
    rq = rq.to(dev)
    E = rq.codebooks[0].weight[:-1].detach().cpu().numpy()
    z = synth.z_tokens(E, cfg["B"], cfg["latent"][0], cfg["latent"][1], 4242)
    x = torch.from_numpy(z.transpose(0, 2, 3, 1).copy()).to(dev)
    depth = cfg["code"][-1]
    W = rq.codebooks[0].weight.detach()
    rec = {"case": name, "B": cfg["B"], "latent": list(cfg["latent"]), "code": list(cfg["code"]), "K": cfg["K"],
           "N": cfg["B"] * cfg["latent"][0] * cfg["latent"][1]}
    if cfg["train"]:
        rq.eval()                             # (fixed codebooks: every iteration times the same work; the EMA is not what is timed)
        R = torch.randn_like(x)
        xg = x.clone().requires_grad_(True)

        def op():
            out, loss, _ = rq(xg)
            ((out * R).sum() + loss).backward()

        def ref():
            out, loss, _ = torch_ops(xg, W, depth)
            ((out * R).sum() + loss).backward()
        rec["op_ms"] = median_ms(op, iters, warmup)
        rec["torch_ms"] = median_ms(ref, iters, warmup)
    else:
        rq.eval()
        with torch.no_grad():
            out, loss, codes = rq(x)
            o2, l2, c2 = torch_ops(x, W, depth)
            rec["codes_match_torch_ops_fraction"] = float((codes.reshape(-1, depth) == c2).double().mean())
            rec["op_ms"] = median_ms(lambda: rq(x), iters, warmup)
            rec["get_codes_ms"] = median_ms(lambda: rq.get_codes(x), iters, warmup)
            rec["torch_ms"] = median_ms(lambda: torch_ops(x, W, depth), iters, warmup)
            rec["per_depth"] = split(rq, x, iters, warmup)
    rec["speedup"] = round(rec["torch_ms"] / rec["op_ms"], 2)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
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
            json.dump({"tool": "tools/rq_time.py", "iters": a.iters, "warmup": a.warmup, "hbm_ceiling_bytes_per_s": HBM,
                       "cases": recs}, f, indent=1)


if __name__ == "__main__":
    main()
