"""Golden data of GumbelQuantize, from the reference's own module on the CPU (needs a checkout of the reference, imported
read-only through oracle.refimport; the tests read only the .npz file this writes): tests/golden/gumbel_quantize_B2.npz.

Stored: the inputs z, W, b, E of the case "golden" of tests/_gumbel_ref.py (B = 2, C = 64, 6 x 6, K = 200, d = 16), the Exp(1)
variates q the reference drew (captured by patching Tensor.exponential_ during its forward at tau = 1.0; the forward at tau = 0.5
is fed the same q the same way), and per tau the reference's z_q, diff, ind.  `meta` (JSON): err_ref, margin = 8 * err_ref, the
share of tokens the near-tie rule leaves out per case.

Checked here, for EVERY case of tests/_gumbel_ref.py (the others are regenerated from their seeds, here and in the tests):
  * err_ref = max |s_f32 - s_f64| of the scores (logits - log q) / tau, s_f32 from the reference's own torch ops on the CPU;
  * tests/_gumbel_ref.py reproduces the reference's `ind` wherever the float64 top-2 gap exceeds the margin, and the tokens left
    out are at most 2 % of the case (else: pick other seeds);
  * its KL term is within 1e-5 relative of the reference's diff / kl_weight, its z_q within 2^-22 relative of the reference's.

    python tools/gen_golden_gumbel.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimport  # noqa: E402
from tests import _gumbel_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", R.FIXTURE)


def reference_class():
    refimport.setup()
    from modules.vector_quantization.quantize_vqgan import GumbelQuantize
    return GumbelQuantize


class patched_exponential:
    """Tensor.exponential_ records what it drew (feed None) or fills in `feed`"""

    def __init__(self, feed=None):
        self.feed, self.seen = feed, []

    def __enter__(self):
        self.orig = orig = torch.Tensor.exponential_
        me = self

        def exponential_(t, *a, **kw):
            if me.feed is None:
                orig(t, *a, **kw)
            else:
                t.copy_(me.feed)
            me.seen.append(t.detach().clone())
            return t
        torch.Tensor.exponential_ = exponential_
        return self

    def __exit__(self, *exc):
        torch.Tensor.exponential_ = self.orig
        return False


def run_case(name, cls, seed_torch):
    B, C, H, Wd, K, d, _ = R.CASES[name]
    z, W, b, E, q = R.case_inputs(name)
    m = cls(C, d, K).eval()
    with torch.no_grad():
        m.proj.weight.copy_(torch.from_numpy(W).reshape(K, C, 1, 1))
        m.proj.bias.copy_(torch.from_numpy(b))
        m.embed.weight.copy_(torch.from_numpy(E))
    zt = torch.from_numpy(z)
    rec, err, shares = {}, 0.0, {}
    for i, tau in enumerate(R.TAUS):
        with torch.no_grad():
            if name == "golden" and i == 0:            # the reference's own draw
                torch.manual_seed(seed_torch)
                with patched_exponential() as pe:
                    zq, diff, (_, _, ind) = m(zt, temp=tau)
                assert len(pe.seen) == 1 and tuple(pe.seen[0].shape) == (B, K, H, Wd)
                q = pe.seen[0].numpy().copy()
                assert (q > 0).all()
            else:
                with patched_exponential(torch.from_numpy(q)) as pe:
                    zq, diff, (_, _, ind) = m(zt, temp=tau)
                assert len(pe.seen) == 1
            s32 = ((m.proj(zt) + (-torch.from_numpy(q).log())) / tau).numpy()
        s64, codes, kl, zq64 = R.forward(z, W, b, E, q, tau)
        err = max(err, float(np.abs(s32.astype(np.float64) - s64).max()))
        rec[tau] = dict(zq=zq.numpy(), diff=np.float32(diff.item()), ind=ind.numpy(), s64=s64, codes=codes, kl=kl, zq64=zq64)
        assert ind.dtype == torch.int64 and tuple(ind.shape) == (B, H, Wd)
    return (z, W, b, E, q), m, rec, err


def main():
    cls = reference_class()
    runs = {name: run_case(name, cls, 91) for name in R.CASES}
    err_ref = max(r[3] for r in runs.values())
    margin = 8.0 * err_ref
    shares = {}
    for name, (inp, m, rec, _) in runs.items():
        for tau, r in rec.items():
            keep = R.top2_gap(r["s64"]) > margin
            share = 1.0 - float(keep.mean())
            shares["%s@%g" % (name, tau)] = share
            assert share <= R.SKIP_CAP, "%s tau %g: %.4f of the tokens are near-ties: pick another seed" % (name, tau, share)
            assert np.array_equal(r["codes"][keep], r["ind"][keep]), "%s tau %g: restatement != reference away from near-ties" % (name, tau)
            want = float(r["diff"]) / m.kl_weight
            assert abs(r["kl"] - want) <= 1e-5 * abs(want), (name, tau, r["kl"], want)
            same = np.broadcast_to((r["codes"] == r["ind"])[:, None], r["zq"].shape)
            assert (np.abs(r["zq"] - r["zq64"])[same] <= 2.0 ** -22 * np.abs(r["zq"])[same]).all(), (name, tau)
            print("%-7s tau %-4g N %5d  left out %.5f  KL %.6f (reference %.6f)" % (name, tau, keep.size, share, r["kl"], want))
    (z, W, b, E, q), m, rec, _ = runs["golden"]
    meta = dict(err_ref=err_ref, margin=margin, factor=8, taus=list(R.TAUS), kl_weight=m.kl_weight, left_out=shares,
                state_keys=sorted(m.state_dict().keys()), torch_seed=91)
    out = dict(z=z, W=W, b=b, E=E, q=q, meta=np.array(json.dumps(meta)))
    for i, tau in enumerate(R.TAUS):
        out.update({"zq%d" % i: rec[tau]["zq"], "diff%d" % i: rec[tau]["diff"], "ind%d" % i: rec[tau]["ind"]})
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    assert size < (1 << 20), size
    print("err_ref %.3e  margin %.3e  %s: %d bytes" % (err_ref, margin, os.path.relpath(OUT, ROOT), size))


if __name__ == "__main__":
    main()
