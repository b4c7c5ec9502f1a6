"""Golden data of MaskVectorQuantize / VectorQuantize, from the reference's own modules on the CPU (needs a checkout of the
reference, imported read-only through oracle.refimport; the tests read only the .npz files this writes).

Per fixture: seeded synth inputs -> the reference module's forward at temp = 0 and, where listed, at a temp > 0 under
torch.manual_seed(seed).  The uniforms of that forward are recovered by re-seeding and replaying torch.zeros(N, K).uniform_(0, 1):
the generator asserts that gumbel_sample of the reference's own `dist` with THAT u gives the forward's codes.  `dist` is rebuilt
with the reference's expressions on the reference's layout (and asserted to give the forward's temp = 0 codes).

Fixtures (tests/_maskvq_ref.py: FIXTURES, tests/test_maskvq.py):
  a_l2_masked  MaskVectorQuantize D = 256, K = 96, NCHW B = 2, 8 x 8, codebook_mask; temp 0 and 1.0   (three code tiles)
  b_l2_flat    MaskVectorQuantize D = 64, K = 1024, channel_last [1, 200, 64]; temp 0 and 0.5         (N % 32, N % 128 != 0)
  c_cosine     MaskVectorQuantize use_cosine_sim D = 128, K = 160, NCHW B = 2, 7 x 9; temp 0 and 1.0; the normalised operands too
  d_ties_l2 / d_ties_cos   K = 96, D = 64, 40 rows: duplicated codebook rows, tokens equal to a code, a NaN token, a zero token; temp 0
  e_cosdist    VectorQuantize use_cosine_distance D = 64, K = 64, [B, D, N] = [2, 64, 50]; temp 0 and 1.0

Checked here: G_ERR (tests/_maskvq_ref.py) bounds |fp32 torch chain - float64 chain| of the gumbel noise of every stored u; the
restatement reproduces the reference's codes outside the skip set, which holds at most 0.1 % of the tokens (else: another seed).

    python tools/gen_golden_maskvq.py
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle, refimport  # noqa: E402
from dynamicvectorquantization_amd import synth  # noqa: E402
from tests import _maskvq_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIDE_BYTES = 256 << 10
PART_BYTES = 720 << 10
G_SEEN = [0.0]


def classes():
    refimport.setup()
    from modules.vector_quantization.quantize_codebook_mask import MaskVectorQuantize
    from modules.vector_quantization.quantize import VectorQuantize
    import modules.vector_quantization.common_utils as utils
    return MaskVectorQuantize, VectorQuantize, utils


def rows_of(x, layout):
    """the reference's `flatten` [N, D] of the module input"""
    if layout == "nchw":
        b, c = x.shape[:2]
        return x.reshape(b, c, -1).permute(0, 2, 1).contiguous().reshape(-1, c)
    if layout == "bdn":
        return x.permute(0, 2, 1).contiguous().reshape(-1, x.shape[1])
    return x.reshape(-1, x.shape[-1])


def ref_dist(rows, w, metric):
    """the reference's `dist` [N, K] and the operands it was computed from"""
    if metric == "cos":
        a, b = F.normalize(rows.unsqueeze(0), p=2, dim=-1), F.normalize(w, p=2, dim=-1).unsqueeze(0)
        return torch.einsum('h n d, h c d -> h n c', a, b)[0], a[0], b[0]
    if metric == "cosdist":
        a, b = F.normalize(rows.unsqueeze(0), p=2, dim=-1).view(-1, rows.shape[1]), F.normalize(w, p=2, dim=-1)
    else:
        a, b = rows, w
    d = - torch.sum(a ** 2, dim=1, keepdim=True) - torch.sum(b ** 2, dim=1) + 2 * torch.einsum('bd,dn->bn', a, b.t())
    return d, a, b


def fixture(tag, cls_name, kw, layout, metric, E, x, mask, temp1, seed):
    Mask, Plain, utils = classes()
    cls = Mask if cls_name == "mask" else Plain
    K, D = E.shape
    m = cls(K, D, **kw).eval()
    xt = torch.from_numpy(x)
    mt = None if mask is None else torch.from_numpy(mask)
    rec = dict(cls=np.array(cls_name), layout=np.array(layout), metric=np.array(metric), D=np.int64(D), K=np.int64(K), E=E, x=x,
               beta=np.float32(m.beta), seed=np.int64(seed), state_keys=np.array(sorted(m.state_dict().keys())))
    if mask is not None:
        rec["mask"] = mask

    def fwd(temp):
        args = dict(temp=temp) if mt is None else dict(temp=temp, codebook_mask=mt)
        xq, loss, (_, _, ind) = m(xt, **args)
        return xq.numpy(), np.float32(loss.item()), ind.numpy()

    with torch.no_grad():
        m.embedding.weight.copy_(torch.from_numpy(E))
        rows = rows_of(xt, layout)
        dist, a, b = ref_dist(rows, m.embedding.weight, metric)
        dn = dist.numpy()
        N = rows.shape[0]
        xq0, loss0, codes0 = fwd(0.)
        assert np.array_equal(R.argmax_torch(dn), codes0.reshape(-1)), "%s: dist does not give the forward's codes" % tag
        assert np.array_equal(torch.argmax(dist, dim=-1).numpy(), codes0.reshape(-1))
        rec.update(dist=dn, xq0=xq0, loss0=loss0, codes0=codes0)
        if metric != "l2":
            rec.update(xn=a.numpy(), wn=b.numpy())
        else:
            od = np.stack([oracle.token_distances(rows[n].numpy(), E) for n in range(N)])
            fin = np.isfinite(od).all(axis=1)
            rec["dist_bits_equal_oracle"] = np.array(bool(np.array_equal((-od[fin]).view(np.uint32), dn[fin].view(np.uint32))))
        share = 0.0
        if temp1 is not None:
            for attempt in range(20):
                torch.manual_seed(seed + attempt)
                xq1, loss1, codes1 = fwd(temp1)
                torch.manual_seed(seed + attempt)
                u = torch.zeros(N, K).uniform_(0, 1)
                g32 = -utils.log(-utils.log(u))
                again = ((dist / temp1) + g32).argmax(dim=-1)
                assert torch.equal(again, torch.from_numpy(codes1.reshape(-1))), "%s: replayed u is not the forward's noise" % tag
                un = u.numpy()
                G_SEEN[0] = max(G_SEEN[0], float(np.abs(g32.numpy().astype(np.float64) - R.gumbel64(un)).max()))
                skip = R.skip_sampled(dn, temp1, un)
                keep = ~skip
                mine = R.argmax_torch(R.perturbed(dn, temp1, un))
                share = float(skip.mean())
                if share <= R.SKIP_CAP and np.array_equal(mine[keep], codes1.reshape(-1)[keep]):
                    break
            else:
                raise AssertionError("%s: no seed keeps the skip set under the cap" % tag)
            rec.update(temp1=np.float32(temp1), seed1=np.int64(seed + attempt), u1=un, xq1=xq1, loss1=loss1, codes1=codes1, skip1=skip)
    for f in os.listdir(OUT):
        if f.startswith("maskvq_%s." % tag):
            os.remove(os.path.join(OUT, f))
    for field in R.SIDE_FIELDS:
        arr = rec.get(field)
        if arr is not None and arr.nbytes > SIDE_BYTES:
            n_rows = max(1, PART_BYTES // (arr.nbytes // arr.shape[0]))
            parts = [arr[i:i + n_rows] for i in range(0, arr.shape[0], n_rows)]
            for i, part in enumerate(parts):
                np.savez_compressed(os.path.join(OUT, "maskvq_%s.%s%d.npz" % (tag, field, i)), a=part)
            rec[field + "_parts"] = np.int64(len(parts))
            del rec[field]
    np.savez_compressed(os.path.join(OUT, "maskvq_%s.npz" % tag), **rec)
    sizes = [os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("maskvq_%s." % tag)]
    assert max(sizes) < (1 << 20), sizes
    print("%s: N %d  skip share %.5f  files %d, largest %d bytes%s" % (
        tag, N, share, len(sizes), max(sizes),
        "" if "dist_bits_equal_oracle" not in rec else "  dist bits == -oracle: %s" % bool(rec["dist_bits_equal_oracle"])))


def nchw(E, B, H, W, seed):
    return synth.z_tokens(E, B, H, W, seed)


def tie_case():
    E = synth.codebook_trained(96, 64, seed=8141).copy()
    E[70], E[33], E[95] = E[5], E[12], E[40]
    x = np.ascontiguousarray(synth.z_tokens(E, 1, 40, 1, 8142)[0, :, :, 0].T)
    x[0], x[1], x[4] = E[70], E[33], E[95]          # equal to a duplicated code: the first of the pair wins
    x[2, 17] = np.nan                               # every score NaN: the first NaN, index 0
    x[3] = 0.0                                      # the zero token (cosine: every score 0, index 0)
    x[5] = 2.0 * E[70]
    return E, x.reshape(1, 40, 64)


def main():
    E = synth.codebook_trained(96, 256, seed=8101)
    mask = synth.bernoulli(8103, (2, 1, 8, 8), 0.6).astype(np.float32)
    fixture("a_l2_masked", "mask", {}, "nchw", "l2", E, nchw(E, 2, 8, 8, 8102), mask, 1.0, 81)
    E = synth.codebook_trained(1024, 64, seed=8111)
    x = np.ascontiguousarray(synth.z_tokens(E, 1, 200, 1, 8112)[0, :, :, 0].T).reshape(1, 200, 64)
    fixture("b_l2_flat", "mask", dict(accept_image_fmap=False, channel_last=True), "flat", "l2", E, x, None, 0.5, 82)
    E = synth.codebook_trained(160, 128, seed=8121)
    fixture("c_cosine", "mask", dict(use_cosine_sim=True), "nchw", "cos", E, nchw(E, 2, 7, 9, 8122), None, 1.0, 83)
    E, x = tie_case()
    flat = dict(accept_image_fmap=False, channel_last=True)
    fixture("d_ties_l2", "mask", flat, "flat", "l2", E, x, None, None, 84)
    fixture("d_ties_cos", "mask", dict(use_cosine_sim=True, **flat), "flat", "cos", E, x, None, None, 85)
    E = synth.codebook_trained(64, 64, seed=8151)
    x = np.ascontiguousarray(synth.z_tokens(E, 2, 50, 1, 8152)[:, :, :, 0])
    fixture("e_cosdist", "plain", dict(use_cosine_distance=True, accept_image_fmap=False, channel_last=False), "bdn", "cosdist",
            E, x, None, 1.0, 86)
    print("largest |g32 - g64| over the stored u: %r  (tests/_maskvq_ref.py: G_ERR = %r)" % (G_SEEN[0], R.G_ERR))
    assert G_SEEN[0] <= R.G_ERR, "raise G_ERR in tests/_maskvq_ref.py to the measured value"


if __name__ == "__main__":
    main()
