"""Golden data of the fused soft code assignment, from the reference's own ops on the CPU (needs a checkout of the reference,
imported read-only through oracle.refimport; the tests read only the .npz files this writes).

Per case: seeded synth inputs -> the reference's VQEmbedding.compute_distances, F.softmax(-d / temp, dim=-1), argmin, and
torch.multinomial's draw.  The variates: q0 = torch.empty_like(p).exponential_(1) under torch.manual_seed(seed) is what
torch.multinomial(p, 1) draws under the same seed -- the generator asserts that argmax(p / q0) IS multinomial's sample -- and the
fixture keeps q = q0 with the lower 16 mantissa bits cleared (still an fp32 number; half the bytes), with code_draw =
argmax(p / q) by the same two torch ops.

Cases (tests/test_soft_assign.py):
  d256_k96       D = 256, K = 96, N = 200     partial 128-token chunk, three 32-code tiles
  d64_k1024      D = 64, K = 1024, N = 129    one token into a second chunk
  d256_k16384    D = 256, K = 16384, N = 64   the long row: distances not stored, soft as CRC + 4 full rows
  tiestress_k96  D = 256, K = 96, N = 200     default-init codebook U(-1/K, 1/K)
temp = the power of two nearest the median spread of a row's four smallest distances: soft codes neither one-hot nor flat.

Checked here and recorded in each file:
  dist_bits_equal_oracle   the reference's distances equal oracle/dvq_oracle.c's bitwise (asserted at D = 256; recorded at D = 64,
                           where the test pins the oracle's bits if they differ)
  e_ref, soft_tol          e_ref = max |reference fp32 softmax - float64 softmax of the same fp32 distances|, soft_tol = 4 e_ref
                           (one e_ref each for another expf, another summation order, the final division, and slack)
  skip_share               share of tokens whose two best p / q are within 1e-4 relative (float64): must be <= 1 %

    python tools/gen_golden_soft.py
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
from tests import _cases as C  # noqa: E402
from tests import _soft_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
SIDE_BYTES = 256 << 10        # arrays above this go to side files ...
PART_BYTES = 720 << 10        # ... of at most this many bytes each (every committed file stays under 1 MiB)


def codebook(kind, K, D, seed):
    return synth.codebook_trained(K, D, seed=seed) if kind == "trained" else synth.codebook_default_init(K, D, seed=seed)


def inputs(E, N, seed):
    z = synth.z_tokens(E, 1, N, 1, seed)                          # [1, D, N, 1]
    return np.ascontiguousarray(z[0, :, :, 0].T)                  # [N, D]


def case(tag, kind, D, K, N, seed, store_dist=True, soft_rows=None):
    refimport.setup()
    from modules.vector_quantization.quantize2_mask import VQEmbedding
    E = codebook(kind, K, D, 7400 + seed)
    x = inputs(E, N, 7500 + seed)
    cb = VQEmbedding(K, D)
    with torch.no_grad():
        cb.weight[:-1].copy_(torch.from_numpy(E))
        d = cb.compute_distances(torch.from_numpy(x))
        dn = d.numpy()
        srt = np.sort(dn, axis=1)
        spread = float(np.median(srt[:, 3] - srt[:, 0]))
        temp = float(2.0 ** np.clip(np.round(np.log2(max(spread, 1e-30))), -20, 20))
        p = F.softmax(-d / temp, dim=-1)
        code_hard = torch.argmin(d, dim=-1)
        torch.manual_seed(seed)
        q0 = torch.empty_like(p).exponential_(1)
        torch.manual_seed(seed)
        drawn = torch.multinomial(p, 1).reshape(-1)
        assert torch.equal(torch.argmax(p / q0, dim=-1), drawn), "q0 is not multinomial's draw"
        qbits = (q0.numpy().view(np.uint32) >> np.uint32(16)).astype(np.uint16)
        q = torch.from_numpy(R.q_from_bits(qbits))
        assert float(q.min()) > 0.0
        code_draw = torch.argmax(p / q, dim=-1)
    od = np.stack([oracle.token_distances(x[n], E) for n in range(N)])
    bits_equal = bool(np.array_equal(od.view(np.uint32), dn.view(np.uint32)))
    if D == 256:
        assert bits_equal, "reference distances differ from the CPU oracle at D = 256"
    pn = p.numpy()
    p64 = R.softmax64(dn, temp)
    e_ref = float(np.abs(pn.astype(np.float64) - p64).max())
    skip = R.skip_set(p64, q.numpy())
    skip_share = float(skip.mean())
    assert skip_share <= 0.01, "%s: %.3f of the tokens draw within 1e-4: choose another seed / temp" % (tag, skip_share)
    pmax = pn.max(axis=1)
    assert np.median(pmax) < 0.999 and np.median(pmax) > 4.0 / K, "%s: soft codes one-hot or flat (median max %g)" % (tag, np.median(pmax))
    rec = dict(D=np.int64(D), K=np.int64(K), N=np.int64(N), seed=np.int64(seed), cb_kind=np.array(kind), cb_seed=np.int64(7400 + seed),
               cb_crc=C.crc(E), x=x, temp=np.float32(temp), code_hard=code_hard.numpy(), code_draw=code_draw.numpy(),
               dist_bits_equal_oracle=np.array(bits_equal), oracle_dist_crc=C.crc(od), e_ref=np.float64(e_ref),
               soft_tol=np.float64(4.0 * e_ref), skip_share=np.float64(skip_share), soft_crc=C.crc(pn), qbits=qbits)
    if store_dist:
        rec["dist"] = dn
        if not bits_equal:
            rec["dist_oracle"] = od                                 # what the GPU test pins when the reference's bits differ
    if soft_rows is None:
        rec["soft"] = pn
    else:
        rec["soft_rows_idx"] = np.array(soft_rows, np.int64)
        rec["soft_rows"] = pn[list(soft_rows)]
    for f in os.listdir(OUT):
        if f.startswith("soft_assign_%s." % tag):
            os.remove(os.path.join(OUT, f))
    for field in ("dist", "dist_oracle", "soft", "qbits"):
        a = rec.get(field)
        if a is not None and a.nbytes > SIDE_BYTES:
            rows = max(1, PART_BYTES // (a.nbytes // a.shape[0]))
            parts = [a[i:i + rows] for i in range(0, a.shape[0], rows)]
            for i, part in enumerate(parts):
                np.savez_compressed(os.path.join(OUT, "soft_assign_%s.%s%d.npz" % (tag, field, i)), a=part)
            rec[field + "_parts"] = np.int64(len(parts))
            del rec[field]
    path = os.path.join(OUT, "soft_assign_%s.npz" % tag)
    np.savez_compressed(path, **rec)
    sizes = [os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("soft_assign_%s." % tag)]
    assert max(sizes) < (1 << 20), sizes
    print("%s: temp %g  e_ref %.3g  soft_tol %.3g  skip_share %.4f  dist bits == oracle: %s  files %d, largest %d bytes"
          % (tag, temp, e_ref, 4 * e_ref, skip_share, bits_equal, len(sizes), max(sizes)))


def main():
    case("d256_k96", "trained", 256, 96, 200, 11)
    case("d64_k1024", "trained", 64, 1024, 129, 12)
    case("d256_k16384", "trained", 256, 16384, 64, 13, store_dist=False, soft_rows=(0, 21, 42, 63))
    case("tiestress_k96", "default", 256, 96, 200, 14)


if __name__ == "__main__":
    main()
