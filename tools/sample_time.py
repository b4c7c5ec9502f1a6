"""Stage-2 sampling glue: the fused head and transfer (csrc/sample.hip) against torch-op forms of the reference's code.
CUDA events, median of --iters after --warmup.  Per (B, V) in {256, 16} x {1258, 2026}, one coarse-position step
(history of 128 positions, top_k 100, top_p 0.9, a draw):
  head_ref_loops   the reference's ops with its per-row Python loops (avoid_repeat_or_enforce_pad_for_coarse_position,
                   dqtransformer_class.py:518-530), then top_k_logits, softmax, top_p_logits, torch.multinomial
  head_torch_vec   the same ops vectorised without the loops (tests/_sample_ref.py: the honest torch baseline)
  head_fused       sample_step: one kernel, q drawn on the device
Per B: the coarse -> fine transfer (~half the cells sampled), the reference's double loop with its per-element host reads
against the count + fill kernels; and a whole sample_from_scratch with the stub transformer of tests/_sample_ref.py
(coarse 4 x 4, fine 8 x 8), the restated torch-op loop against FusedSampling.  One JSON line per number, the record to --out.

    python tools/sample_time.py [--iters 20] [--warmup 3] [--out profiles/sample.json]
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from dynamicvectorquantization_amd.sample import (FusedSampling, SamplingRules, sample_step,  # noqa: E402
                                                  transfer_sampled_coarse_position_to_sampled_fine_position)
from tests import _sample_ref as R  # noqa: E402

CODES = dict(content_pad_code=1024, content_eos_code=1025, coarse_position_pad_code=256, coarse_position_eos_code=257,
             coarse_position_sos_code=258, fine_position_pad_code=1024, fine_position_eos_code=1025, fine_position_sos_code=1026,
             max_coarse_postion_idx=255, hw1=16, fine_hw=32)


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


def loop_mask(logits, hist, flag, c):
    """the per-row loop form of the reference's coarse-position helper"""
    out = logits.clone()
    for i in range(logits.size(0)):
        if flag[i] == 0:
            out[i, hist[i]] = -float("inf")
            out[i, c["coarse_position_pad_code"]] = -float("inf")
            out[i, c["max_coarse_postion_idx"]:] = -float("inf")
            out[i, c["coarse_position_eos_code"]] = logits[i, c["coarse_position_eos_code"]]
        else:
            out[i, :] = -float("inf")
            out[i, c["coarse_position_pad_code"]] = logits[i, c["coarse_position_pad_code"]]
    return out


def head_ref_loops(lg, hist, flag, c, k, p):
    x = lg[:, -1, :] / 1.0
    x = loop_mask(x, hist, flag, c)
    x = R.top_k(x, k)
    probs = torch.softmax(x, -1)
    probs = R.top_p(probs, p)
    return torch.multinomial(probs, 1)


def transfer_ref_loop(cp, c):
    """the reference's double loop (one host read per coarse step) and per-row list + pad_sequence"""
    from torch.nn.utils.rnn import pad_sequence
    B, hw1 = cp.size(0), c["hw1"]
    seq = torch.arange(c["fine_hw"] ** 2).view(hw1, 2, hw1, 2).permute(0, 2, 1, 3).reshape(hw1, hw1, 4)
    pos = cp[:, 1:]
    grain = torch.zeros(B, hw1 * hw1).long()
    for i in range(B):
        for l in range(pos.size(1)):
            if pos[i, l] == c["coarse_position_eos_code"]:
                break
            grain[i, pos[i, l]] = 1
    grain = grain.view(B, hw1, hw1)
    rows = [torch.cat([seq[grain[i] == 1].view(-1).to(cp.device), torch.tensor([c["fine_position_eos_code"]], device=cp.device)])
            for i in range(B)]
    out = pad_sequence(rows, batch_first=True, padding_value=c["fine_position_pad_code"])
    return torch.cat([torch.full((B, 1), c["fine_position_sos_code"], device=cp.device), out], 1)


class _Stub(FusedSampling):
    def __init__(self, c):
        for k, v in R.model_attrs(c, "class", "region-first").items():
            setattr(self, k, v)
        self.transformer = R.StubTransformer(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sample.json"))
    ap.add_argument("--only-fused", action="store_true", help="only the fused head at B = 256, V = 2026 (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    c = CODES
    rules = SamplingRules("class", **{k: v for k, v in c.items() if k != "coarse_position_sos_code"},
                          fine_position_order="region-first")
    rec = {"device": torch.cuda.get_device_name(0), "iters": a.iters, "warmup": a.warmup, "results": []}

    def emit(**kw):
        rec["results"].append(kw)
        print(json.dumps(kw), flush=True)

    g = torch.Generator(device=dev).manual_seed(0)
    shapes = [(256, 2026)] if a.only_fused else [(B, V) for B in (256, 16) for V in (1258, 2026)]
    for B, V in shapes:
        lg = torch.randn(B, 1, V, device=dev, generator=g) * 3
        hist = torch.cat([torch.full((B, 1), 258, device=dev),
                          torch.stack([torch.randperm(256, device=dev)[:128] for _ in range(B)])], 1)
        flag = (torch.arange(B, device=dev)[:, None] % 5 == 0).float()
        k, p = 100, 0.9
        fused = lambda: sample_step(lg, "coarse_position", rules, history=hist, flag=flag.clone(), top_k=k, top_p=p)
        emit(case="head_fused", B=B, V=V, ms=median_ms(fused, a.iters, a.warmup))
        if a.only_fused:
            continue
        vec = lambda: R.head(lg[:, -1, :], "coarse_position", "class", c, hist, flag, 1.0, k, p, True, None)
        emit(case="head_torch_vec", B=B, V=V, ms=median_ms(vec, a.iters, a.warmup))
        loops = lambda: head_ref_loops(lg, hist, flag, c, k, p)
        emit(case="head_ref_loops", B=B, V=V, ms=median_ms(loops, max(3, a.iters // 4), 1))
    if not a.only_fused:
        for B in (256, 16):
            cp = torch.full((B, 258), 256, dtype=torch.long, device=dev)
            cp[:, 0] = 258
            for b in range(B):
                n = 100 + b % 50
                cp[b, 1:1 + n] = torch.randperm(256, device=dev)[:n]
                cp[b, 1 + n] = 257
            assert torch.equal(transfer_sampled_coarse_position_to_sampled_fine_position(rules, cp), transfer_ref_loop(cp, c))
            emit(case="transfer_fused", B=B, ms=median_ms(lambda: transfer_sampled_coarse_position_to_sampled_fine_position(rules, cp),
                                                          a.iters, a.warmup))
            emit(case="transfer_ref_loop", B=B, ms=median_ms(lambda: transfer_ref_loop(cp, c), 3, 1))
        cs = R.codes_small()
        m = _Stub(cs)
        for B in (256, 16):
            cond = R.conditioning(cs, B, dev)
            fl = lambda: m.sample_from_scratch(*cond, top_k=5, top_p=0.9, process=False,
                                               generator=torch.Generator(device=dev).manual_seed(1))
            emit(case="loop_fused_stub", B=B, ms=median_ms(fl, 5, 1))
            rl = lambda: R.sample_loop(R.namespace(cs, "class", "region-first"), "class", cs, cond, 1.0, True, 5, 0.9, None, None,
                                       False, generator=torch.Generator(device=dev).manual_seed(1))
            emit(case="loop_torch_vec_stub", B=B, ms=median_ms(rl, 5, 1))
    if a.out and not a.only_fused:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)


if __name__ == "__main__":
    main()
