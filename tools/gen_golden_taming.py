"""Golden data of VectorQuantizer, EMAVectorQuantizer and the sequence VectorQuantizer2, from the reference's own modules on the
CPU (needs a checkout of the reference, imported read-only through oracle.refimport; the tests read only the .npz files this
writes): tests/golden/taming_{a,b,n,seq}.npz.  Data only: the inputs are regenerated from their seeds (tests/_taming_ref.py), the
files hold their CRCs and the reference's results.

Per class case (tests/_taming_ref.py: CASES):
  vq_*      VectorQuantizer forward + backward of (z_q * gw).sum() + 5 loss: codes, loss, perplexity, CRC of the one-hot matrix,
            z.grad, embedding.weight.grad
  ema_*     EMAVectorQuantizer in eval mode: codes, loss, perplexity, CRC of the one-hot matrix
  step_*    ... one training step from cluster_size = cs0 > 0 (so the smoothing is exercised), embed_avg = E * cs0: outputs as
            above, cluster_size afterwards in full, embed_avg / weight afterwards at `step_rows` (every row a token chose + the
            first 32; the full [K, D] arrays would not fit the size limit)
  noupd_*   ... training mode with embedding.update = False: asserted here to equal eval and to leave the parameters alone
and for the sequence class: codes, loss, z_q CRC.

Asserted here, per case (a failure means: stop, do not loosen a test):
  * the reference's codes equal oracle.vq_assign_nchw's, all of them, and its z_q the oracle's bit for bit;
  * tests/_taming_ref.py reproduces the reference's perplexity within 1e-5 relative, its p_j are mean(one_hot, 0) bit for bit,
    and its float64 EMA step agrees with ALL rows of the reference's post-step parameters within 1e-5 of the largest entry.

    python tools/gen_golden_taming.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle, refimport  # noqa: E402
from tests import _taming_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _rel(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(1e-30, np.abs(want).max()))


def check_stats(tag, codes, K, perplexity, encodings):
    s = R.flat_stats(codes, K)
    enc = encodings.numpy()
    assert np.array_equal(enc, R.onehot(codes, K)), tag
    p32 = s["counts"].astype(np.float32) / np.float32(codes.size)
    assert np.array_equal(_bits(p32), _bits(torch.mean(encodings, dim=0).numpy())), tag + ": p_j != mean(one_hot, 0)"
    ref = float(perplexity)
    for key in ("perplexity", "perplexity_f32"):
        assert abs(s[key] - ref) <= 1e-5 * abs(ref), (tag, key, s[key], ref)
    return dict(perplexity=np.float32(ref), onehot_crc=R.crc(enc), n_used=np.int64(s["n_used"]),
                dev=max(abs(s[k] - ref) / abs(ref) for k in ("perplexity", "perplexity_f32")))


def check_assign(tag, z, E, codes, zq, loss, beta, legacy):
    B = z.shape[0]
    o = oracle.vq_assign_nchw(z, E, None)
    assert np.array_equal(o["codes"], np.asarray(codes).reshape(B, -1)), tag + ": the reference's codes are not the oracle's"
    assert np.array_equal(_bits(o["zq"]).reshape(-1), _bits(zq).reshape(-1)), tag + ": z_q differs from the oracle's"
    return o


def run_class_case(name, VQ, EMA):
    B, D, H, W, K = R.CASES[name]
    z, E, gw, cs0 = R.case_inputs(name)
    N = B * H * W
    out = dict(z_crc=R.crc(z), E_crc=R.crc(E), gw_crc=R.crc(gw), cs0_crc=R.crc(cs0), shape=np.array([B, D, H, W, K], np.int64))
    devs = {}
    # ---- VectorQuantizer, forward + backward
    m = VQ(K, D, R.BETA)
    with torch.no_grad():
        m.embedding.weight.copy_(torch.from_numpy(E))
    zt = torch.from_numpy(z).requires_grad_(True)
    zq, loss, (perp, enc, idx) = m(zt)
    ((zq * torch.from_numpy(gw)).sum() + 5.0 * loss).backward()
    codes = idx.numpy().reshape(-1)
    assert tuple(idx.shape) == (N, 1) and tuple(enc.shape) == (N, K) and enc.dtype == torch.float32
    o = check_assign("vq_" + name, z, E, codes, zq.detach().numpy(), float(loss), R.BETA, True)
    want = oracle.vq_loss(o["sqerr"], o["numel"], R.BETA, legacy=True)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    st = check_stats("vq_" + name, codes, K, perp, enc.detach())
    devs["vq"] = st.pop("dev")
    out.update({"vq_" + k: v for k, v in st.items()})
    out.update(vq_codes=codes.astype(np.int32), vq_loss=np.float32(loss.item()), vq_zq_crc=R.crc(zq.detach().numpy()),
               vq_z_grad=zt.grad.numpy(), vq_w_grad=m.embedding.weight.grad.numpy(),
               vq_state_keys=np.array(json.dumps(sorted(m.state_dict().keys()))))

    # ---- EMAVectorQuantizer: eval, update = False, one training step
    def make():
        e = EMA(K, D, R.BETA, decay=R.DECAY, eps=R.EPS)
        with torch.no_grad():
            e.embedding.weight.copy_(torch.from_numpy(E))
            e.embedding.cluster_size.copy_(torch.from_numpy(cs0))
            e.embedding.embed_avg.copy_(torch.from_numpy(E * cs0[:, None]))
        return e

    def fwd(e):
        zt = torch.from_numpy(z).requires_grad_(True)
        zq, loss, (perp, enc, idx) = e(zt)
        ((zq * torch.from_numpy(gw)).sum() + 5.0 * loss).backward()
        assert tuple(idx.shape) == (N,) and tuple(enc.shape) == (N, K)
        return zq.detach().numpy(), float(loss), perp, enc.detach(), idx.numpy(), zt.grad.numpy()

    e = make().eval()
    zq, loss, perp, enc, codes, zgrad = fwd(e)
    o = check_assign("ema_" + name, z, E, codes, zq, loss, R.BETA, True)
    mse = float(o["sqerr"]) / o["numel"]
    assert abs(loss - R.BETA * mse) <= 1e-5 * R.BETA * mse
    st = check_stats("ema_" + name, codes, K, perp, enc)
    devs["ema"] = st.pop("dev")
    out.update({"ema_" + k: v for k, v in st.items()})
    out.update(ema_codes=codes.astype(np.int32), ema_loss=np.float32(loss), ema_zq_crc=R.crc(zq), ema_z_grad=zgrad,
               ema_state_keys=np.array(json.dumps(sorted(e.state_dict().keys()))),
               ema_state_shapes=np.array(json.dumps({k: list(v.shape) for k, v in e.state_dict().items()})))
    e2 = make().train()
    e2.embedding.update = False
    zq2, loss2, perp2, enc2, codes2, _ = fwd(e2)
    assert np.array_equal(codes2, codes) and np.array_equal(_bits(zq2), _bits(zq)) and loss2 == loss and float(perp2) == float(perp)
    assert np.array_equal(e2.embedding.weight.numpy(), E) and np.array_equal(e2.embedding.cluster_size.numpy(), cs0)
    e3 = make().train()
    zq3, loss3, perp3, enc3, codes3, _ = fwd(e3)
    assert np.array_equal(codes3, codes) and np.array_equal(_bits(zq3), _bits(zq)) and loss3 == loss     # the OLD weight
    cs, avg, w = R.ema_step(z, codes3, cs0, E * cs0[:, None])
    got = (e3.embedding.cluster_size.numpy(), e3.embedding.embed_avg.numpy(), e3.embedding.weight.numpy())
    devs["step"] = max(_rel(g, r) for g, r in zip(got, (cs, avg, w)))
    assert devs["step"] < 1e-5, devs["step"]
    rows = np.unique(np.concatenate([np.arange(min(32, K)), codes3])).astype(np.int64)
    out.update(step_rows=rows.astype(np.int32), step_cluster_size=got[0], step_embed_avg=got[1][rows], step_weight=got[2][rows])
    out["meta"] = np.array(json.dumps(dict(beta=R.BETA, decay=R.DECAY, eps=R.EPS, torch=torch.__version__, loss_weight=5.0,
                                           deviation={k: float(v) for k, v in devs.items()})))
    return out, devs


def run_seq(Seq):
    B, D, L, K = R.SEQ
    z, E = R.seq_inputs()
    out = dict(z_crc=R.crc(z), E_crc=R.crc(E), shape=np.array([B, D, L, K], np.int64))
    for legacy in (True, False):
        m = Seq(K, D, R.BETA, legacy=legacy)
        with torch.no_grad():
            m.embedding.weight.copy_(torch.from_numpy(E))
        zt = torch.from_numpy(z)
        with torch.no_grad():
            zq, loss, (p, e, idx) = m(zt)
        assert p is None and e is None and tuple(idx.shape) == (B * L,) and tuple(zq.shape) == (B, D, L)
        o = check_assign("seq", z, E, idx.numpy(), zq.numpy(), float(loss), R.BETA, legacy)
        want = oracle.vq_loss(o["sqerr"], o["numel"], R.BETA, legacy=legacy)
        assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want))
        s = "_legacy%d" % int(legacy)
        out.update({"codes" + s: idx.numpy().astype(np.int32), "loss" + s: np.float32(loss.item()), "zq_crc" + s: R.crc(zq.numpy())})
        entry = m.get_codebook_entry(idx, (B, L, D))
        assert tuple(entry.shape) == (B, D, L)
        out["entry_crc"] = R.crc(entry.detach().numpy())
    out["state_keys"] = np.array(json.dumps(sorted(m.state_dict().keys())))
    return out


def main():
    refimport.setup()
    oracle.build()
    from modules.vector_quantization.quantize_vqgan import EMAVectorQuantizer, VectorQuantizer
    from modules.vqvae.quantize2 import VectorQuantizer2 as Seq
    torch.manual_seed(0)
    for name in sorted(R.CASES):
        out, devs = run_class_case(name, VectorQuantizer, EMAVectorQuantizer)
        path = os.path.join(GOLDEN, R.GOLDEN_FILE % name)
        np.savez_compressed(path, **out)
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print("%-3s %s  perplexity vq %.6f ema %.6f  deviations %s  %d bytes" % (
            name, R.CASES[name], float(out["vq_perplexity"]), float(out["ema_perplexity"]),
            {k: "%.2e" % v for k, v in devs.items()}, size))
    out = run_seq(Seq)
    path = os.path.join(GOLDEN, R.GOLDEN_FILE % "seq")
    np.savez_compressed(path, **out)
    print("seq %s  %d bytes" % (R.SEQ, os.path.getsize(path)))


if __name__ == "__main__":
    main()
