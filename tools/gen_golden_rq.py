"""Golden data of residual quantization, from the reference's own RQBottleneck (CPU; needs a checkout of the reference, imported
through oracle.refimport; the tests read only the .npz files this writes).

Cases of tests/test_rq.py:
  eval_shared    latent (8, 8, 256), code (8, 8, 4), one shared codebook of K = 256, B = 2: forward, agg_d (quant_list[-1]),
                 and in rq_eval_shared_embed.npz embed_code, embed_code_with_depth(.., True), embed_partial_code at depth 1
  eval_separate  latent (8, 8, 64), code (4, 4, 4): divisor 2, D = 256, codebooks n_embed = [64, 128, 128, 256], list decay
  train_shared   one training step, restart_unused_codes=False, shared K = 64 (N = 128), loss sum(out * R) + 3 * loss:
                 x.grad and every codebook's cluster_size_ema / embed_ema / weight after the step
  train_separate the same with separate codebooks [32, 64, 128] at divisor 2 and restart_unused_codes=True (N = 128 >= every K,
                 so _tile_with_noise does not run), torch.randperm replaced by a reversed arange
Cases of tests/test_rq_shapes.py (every third channel of every fifth codebook row and every seventh element of x are -0.0 in the
eval cases, so that the sign rules of fl(0 + e) and fl(x + fl(agg - x)) show; partial embeds at depth min(1, depth - 1)):
  eval_r2x8_dl6  latent (6, 40, 6), code (3, 5, 3), codebooks [40, 72, 100], B = 3: divisor 2 x 8, Dl = 6, D = 96
  eval_r4x2_dl8  latent (20, 6, 8), code (5, 3, 2), codebooks [50, 64], B = 5: divisor 4 x 2, Dl = 8, D = 64
  eval_depth1    latent (3, 7, 32), code (3, 7, 1), shared K = 33, B = 2: depth 1, D = 32
  eval_depth16   latent (4, 6, 16), code (2, 3, 16), shared K = 48, B = 3: depth 16 at divisor 2
  eval_r2x8_dl2  latent (2, 16, 2), code (1, 2, 2), shared K = 20, B = 7: Dl = 2, D = 32, h = 1
  train_r2x4     one training step at latent (6, 20, 8), code (3, 5, 3), shared K = 40 (N = 45), restart off, divisor 2 x 4
Codebooks are synth.codebook_trained (padding row left as the reference initialises it); inputs are synth.z_tokens around codebook
rows, channel-last.  Every file also stores the reference's state_dict key list.

    python tools/gen_golden_rq.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimport  # noqa: E402
from dynamicvectorquantization_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")


def _module(latent, code, n_embed, decay, shared, restart, seed, neg_zero=False):
    refimport.setup()
    from modules.vector_quantization.quantize_rqvae import RQBottleneck
    torch.manual_seed(seed)
    rq = RQBottleneck(latent_shape=latent, code_shape=code, n_embed=n_embed, decay=decay, shared_codebook=shared,
                      restart_unused_codes=restart)
    D = rq.codebooks[0].weight.shape[1]
    with torch.no_grad():
        for i, cb in enumerate(rq.codebooks[:1] if shared else rq.codebooks):
            E = synth.codebook_trained(cb.n_embed, D, seed=1001 + 17 * i)
            if neg_zero:
                E[::5, ::3] = -0.0
            cb.weight[:-1].copy_(torch.from_numpy(E))
            cb.embed_ema.copy_(cb.weight[:-1])
    return rq


def _latents(rq, B, seed):
    """channel-last latents [B, H, W, Dl]: tokens around rows of codebook 0 in code layout, put into latent layout"""
    h, w = rq.code_shape[0], rq.code_shape[1]
    E = rq.codebooks[0].weight[:-1].detach().numpy()
    z = synth.z_tokens(E, B, h, w, seed)                                     # [B, D, h, w]
    zc = torch.from_numpy(np.ascontiguousarray(z.transpose(0, 2, 3, 1)))   # [B, h, w, D]
    return rq.to_latent_shape(zc).contiguous()


def _meta(rq, rec):
    rec["latent_shape"] = np.array(tuple(rq.latent_shape))
    rec["code_shape"] = np.array(tuple(rq.code_shape))
    rec["n_embed"] = np.array(rq.n_embed)
    rec["decay"] = np.array(rq.decay, dtype=np.float64)
    rec["shared"] = np.array(bool(rq.shared_codebook))
    rec["restart"] = np.array(bool(rq.restart_unused_codes))
    rec["state_dict_keys"] = np.array(list(rq.state_dict().keys()))
    for i, cb in enumerate(rq.codebooks[:1] if rq.shared_codebook else rq.codebooks):
        rec["weight.%d" % i] = cb.weight.detach().numpy().copy()


def eval_case(tag, latent, code, n_embed, decay, shared, B, seed, neg_zero=False, code_idx=1):
    rq = _module(latent, code, n_embed, decay, shared, True, seed, neg_zero).eval()
    rec = {}
    _meta(rq, rec)
    x = _latents(rq, B, seed + 100)
    if neg_zero:
        x.view(-1)[::7] = -0.0
    with torch.no_grad():
        out, loss, codes = rq(x)
        quant_list, codes2 = rq.quantize(rq.to_code_shape(x))
        agg = rq.to_latent_shape(quant_list[-1])
        emb = rq.embed_code(codes)
        emb_depth, _ = rq.embed_code_with_depth(codes, to_latent_shape=True)
        sel = rq.embed_partial_code(codes, code_idx, "select")
        add = rq.embed_partial_code(codes, code_idx, "add")
        add_last = rq.embed_partial_code(codes, code[-1] - 1, "add")
    assert torch.equal(codes, codes2)
    rec.update(x=x.numpy(), out=out.numpy(), loss=np.float32(loss.item()), codes=codes.numpy(), agg=agg.numpy(),
               agg_equals_embed_code=np.array(bool(torch.equal(agg, emb))),
               add_last_equals_embed_code=np.array(bool(torch.equal(add_last, emb))))
    emb_rec = {"embed_code": emb.numpy(), "embed_code_with_depth": emb_depth.numpy(), "partial_select_%d" % code_idx: sel.numpy(),
               "partial_add_%d" % code_idx: add.numpy()}
    for name, r in (("rq_%s.npz" % tag, rec), ("rq_%s_embed.npz" % tag, emb_rec)):
        path = os.path.join(OUT, name)
        np.savez_compressed(path, **r)
        print("%s: %d bytes" % (path, os.path.getsize(path)))


def train_case(tag, latent, code, n_embed, shared, restart, B, seed):
    rq = _module(latent, code, n_embed, 0.99, shared, restart, seed).train()
    rec = {}
    _meta(rq, rec)
    x = _latents(rq, B, seed + 100).requires_grad_(True)
    R = torch.from_numpy(synth.normal(seed + 200, tuple(x.shape)))
    orig = torch.randperm
    torch.randperm = lambda n, *a, **kw: torch.arange(n - 1, -1, -1, device=kw.get("device"))
    try:
        out, loss, codes = rq(x)
    finally:
        torch.randperm = orig
    L = (out * R).sum() + 3.0 * loss
    L.backward()
    rec.update(x=x.detach().numpy(), R=R.numpy(), out=out.detach().numpy(), loss=np.float32(loss.item()), codes=codes.numpy(),
               grad_x=x.grad.numpy())
    for i, cb in enumerate(rq.codebooks[:1] if shared else rq.codebooks):
        rec["after.weight.%d" % i] = cb.weight.detach().numpy().copy()
        rec["after.cluster_size_ema.%d" % i] = cb.cluster_size_ema.numpy().copy()
        rec["after.embed_ema.%d" % i] = cb.embed_ema.numpy().copy()
    path = os.path.join(OUT, "rq_%s.npz" % tag)
    np.savez_compressed(path, **rec)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


def main():
    eval_case("eval_shared", (8, 8, 256), (8, 8, 4), 256, 0.99, True, 2, 31)
    eval_case("eval_separate", (8, 8, 64), (4, 4, 4), [64, 128, 128, 256], [0.99, 0.98, 0.97, 0.96], False, 2, 32)
    train_case("train_shared", (8, 8, 64), (8, 8, 4), 64, True, False, 2, 33)
    train_case("train_separate", (8, 8, 32), (4, 4, 3), [32, 64, 128], False, True, 8, 34)
    # tests/test_rq_shapes.py: non-square grids and divisors, Dl % 4 != 0, padded widths, depth 1 / 2 / 16
    eval_case("eval_r2x8_dl6", (6, 40, 6), (3, 5, 3), [40, 72, 100], [0.99, 0.98, 0.97], False, 3, 41, neg_zero=True)
    eval_case("eval_r4x2_dl8", (20, 6, 8), (5, 3, 2), [50, 64], [0.99, 0.98], False, 5, 42, neg_zero=True)
    eval_case("eval_depth1", (3, 7, 32), (3, 7, 1), 33, 0.99, True, 2, 43, neg_zero=True, code_idx=0)
    eval_case("eval_depth16", (4, 6, 16), (2, 3, 16), 48, 0.99, True, 3, 44, neg_zero=True)
    eval_case("eval_r2x8_dl2", (2, 16, 2), (1, 2, 2), 20, 0.99, True, 7, 45, neg_zero=True)
    train_case("train_r2x4", (6, 20, 8), (3, 5, 3), 40, True, False, 3, 46)


if __name__ == "__main__":
    main()
