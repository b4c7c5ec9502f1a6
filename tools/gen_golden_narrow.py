"""Golden data of the narrow widths (codebook_dim 3, 4, 8, 16), from the reference's own modules on the CPU (needs a checkout of
the reference, imported read-only through oracle.refimport; the tests read only the .npz files this writes).

Per width D, cases of seeded synth inputs, each run through
  the reference's quantize2_mask.VectorQuantize2, eval, with a codebook_mask   -> vq2_codes / vq2_zq / vq2_loss
  the reference's quantize_vqgan.VectorQuantizer2, legacy=False                -> vqg_codes / vqg_zq / vqg_loss
Cases (tests/test_narrow_width.py):
  trained   B = 2, 9 x 7, K = 200, a "trained" codebook N(0, 0.5^2), clustered latents
  ties      the same shape, the default-init codebook U(-1/K, 1/K) and latents scaled by 0.002 (tie stress)
  big       D = 4 only: K = 16384, B = 1, 8 x 8
written to tests/golden/narrow_D{3,4,8,16}.npz as <case>_z, <case>_E, <case>_mask and the outputs above.

THE PIN: for every case, and with 1 and with 8 torch threads, oracle.vq_assign_nchw must give the reference's codes with 0
mismatches and its z_q bit for bit, and oracle.token_distances the bits of the reference's own compute_distances for up to 256
tokens of each case (asserted; the counts are printed).  That run is what extends the oracle's validity -- the
sequential-k fmaf chain, dvq_oracle_sumsq, fl(fl(xn + en) - 2 dot), first-index / NaN argmin -- from the multiples of 32 to
these widths.  A width that fails here is not a width the kernels may serve.

    python tools/gen_golden_narrow.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle, refimport  # noqa: E402
from dynamicvectorquantization_amd import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
WIDTHS = (3, 4, 8, 16)
BETA = 0.25
DIST_MISMATCH = [0, 0]                      # (distances whose bits differ from the oracle's, distances compared)


def cases(D):
    """-> [(name, z [B, D, H, W], E [K, D], mask [B, 1, H, W])]"""
    K, B, H, W = 200, 2, 9, 7
    s = 9100 + 10 * D
    out = []
    E = synth.codebook_trained(K, D, seed=s)
    mask = np.where(synth.bernoulli(s + 2, (B, 1, H, W), 0.5), 1.0, 0.25).astype(np.float32)
    out.append(("trained", synth.z_tokens(E, B, H, W, s + 1), E, mask))
    Ed = synth.codebook_default_init(K, D, seed=s + 3)
    out.append(("ties", synth.z_tokens(E, B, H, W, s + 4) * np.float32(0.002), Ed, mask))
    if D == 4:
        Eb = synth.codebook_trained(16384, D, seed=s + 5)
        mb = np.where(synth.bernoulli(s + 7, (1, 1, 8, 8), 0.5), 1.0, 0.25).astype(np.float32)
        out.append(("big", synth.z_tokens(Eb, 1, 8, 8, s + 6), Eb, mb))
    return out


def reference(z, E, mask):
    VQ2, VQG = refimport.quantizers()
    K, D = E.shape
    zt = torch.from_numpy(z)
    with torch.no_grad():
        m = VQ2(K, D, commitment_beta=BETA).eval()
        m.codebook.weight.data[:-1].copy_(torch.from_numpy(E))
        xq, loss, (_, _, codes) = m(zt, codebook_mask=torch.from_numpy(mask))
        rows = zt.permute(0, 2, 3, 1).contiguous().reshape(-1, D)
        dist = m.codebook.compute_distances(rows[:256]).numpy()          # the reference's distance expression itself
        g = VQG(K, D, beta=BETA, legacy=False, sane_index_shape=True).eval()
        g.embedding.weight.data.copy_(torch.from_numpy(E))
        gq, gloss, (_, _, gidx) = g(zt)
    od = np.stack([oracle.token_distances(rows[n].numpy(), E) for n in range(dist.shape[0])])
    DIST_MISMATCH[0] += int((od.view(np.uint32) != np.ascontiguousarray(dist).view(np.uint32)).sum())
    DIST_MISMATCH[1] += dist.size
    return dict(vq2_codes=codes.numpy().astype(np.int64), vq2_zq=xq.numpy(), vq2_loss=np.float32(loss.item()),
                vqg_codes=gidx.numpy().astype(np.int64), vqg_zq=gq.numpy(), vqg_loss=np.float32(gloss.item()))


def bits_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def main():
    failed = []
    for D in WIDTHS:
        rec = {"D": np.int64(D), "beta": np.float32(BETA), "torch": np.array(torch.__version__)}
        names = []
        ok = True
        for name, z, E, mask in cases(D):
            B = z.shape[0]
            first = None
            for threads in (1, 8):
                torch.set_num_threads(threads)
                r = reference(z, E, mask)
                if first is None:
                    first = r
                else:
                    assert all(np.array_equal(first[k], r[k]) for k in ("vq2_codes", "vqg_codes")) and \
                        bits_equal(first["vq2_zq"], r["vq2_zq"]), "the reference differs between 1 and 8 threads"
                om = oracle.vq_assign_nchw(z, E, mask)
                on = oracle.vq_assign_nchw(z, E, None)
                mis2 = int((om["codes"] != r["vq2_codes"].reshape(B, -1)).sum())
                misg = int((on["codes"] != r["vqg_codes"].reshape(B, -1)).sum())
                zq2, zqg = bits_equal(om["zq"], r["vq2_zq"]), bits_equal(on["zq"], r["vqg_zq"])
                print("D %2d %-8s threads %d: VectorQuantize2 %d code mismatches of %d, z_q bit-equal %s; VectorQuantizer2 %d, %s"
                      % (D, name, threads, mis2, om["codes"].size, zq2, misg, zqg))
                ok = ok and mis2 == 0 and misg == 0 and zq2 and zqg
                l2 = float(oracle.vq_loss(om["sqerr"], om["numel"], BETA))
                lg = float(oracle.vq_loss(on["sqerr"], on["numel"], BETA))
                assert abs(l2 - float(r["vq2_loss"])) <= 1e-5 * abs(float(r["vq2_loss"])), (l2, r["vq2_loss"])
                assert abs(lg - float(r["vqg_loss"])) <= 1e-5 * abs(float(r["vqg_loss"])), (lg, r["vqg_loss"])
            names.append(name)
            rec.update({name + "_z": z, name + "_E": E, name + "_mask": mask})
            rec.update({name + "_" + k: v for k, v in first.items()})
        print("D %2d: %d of %d distances of compute_distances differ in bits from oracle.token_distances" % (D, *DIST_MISMATCH))
        ok = ok and DIST_MISMATCH[0] == 0
        DIST_MISMATCH[:] = [0, 0]
        if not ok:
            failed.append(D)
            continue
        rec["cases"] = np.array(names)
        path = os.path.join(OUT, "narrow_D%d.npz" % D)
        np.savez_compressed(path, **rec)
        assert os.path.getsize(path) < (1 << 20)
        print("wrote %s  %.1f KiB" % (os.path.relpath(path, ROOT), os.path.getsize(path) / 1024))
    assert not failed, "widths the oracle does not reproduce bit for bit (they must stay unsupported): %s" % failed


if __name__ == "__main__":
    main()
