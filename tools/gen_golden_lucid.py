"""Golden data of the lucidrains-style quantizer (dynamicvectorquantization_amd/lucid.py), from the reference's own classes on the
CPU (needs a checkout of the reference, imported read-only through oracle.refimport; the tests read only the .npz files this writes).

Fixtures (tests/_lucid_ref.py: FIXTURES, ORTHO_SETS; tests/test_lucid.py):
  a_euclid       VectorQuantize D = 256, K = 96 (three code tiles), NCHW B = 2, 8 x 8, orthogonal_reg_weight 0.5; eval and one training
                 step (decay 0.8, threshold_ema_dead_code 2, picks stored); sample_codebook_temp 0 and 1.0
  b_euclid_flat  VectorQuantize D = 64, K = 1024, channel-last [1, 200, 64] (N % 32 != 0); temp 0 and 0.5; eval and a training step
  c_cosine       CosineSimCodebook direct and as the codebook of a VectorQuantize (the reference's own use_cosine_sim = True raises
                 TypeError: the generator swaps the codebook in), D = 128, K = 160, [2, 63, 128]; eval, training step, expiry
  d_ties         K = 96, D = 64, 40 rows: duplicated codebook rows, tokens equal to a code, a NaN token, a zero token; temp 0, eval
  e_ortho_*      orthogonal_loss_fn in fp32 and float64 with its autograd gradient's fp32 error: n = 96 / D = 64, n = 100 / D = 256,
                 n = 1024 / D = 128, default-init and N(0, 0.5^2) rows, and one set with two duplicated rows and a zero row
  f_kmeans       K = 64, D = 64, N = 512, 3 iterations from stored initial rows, Euclidean and cosine

The reference runs with sync_codebook = False; for expiry its sample_fn is replaced by `samples[:, picks[:num]]` for stored picks.
Checked here: the reference's quantize equals embed[codes] (eval) and fl(x + fl(e - x)) (training) bit for bit, so neither is
stored; embed_avg is unchanged by a training step; argmin of the oracle's distances gives the reference's temp = 0 codes; the
restatement gives its sampled codes outside the skip set (S_ERR measured per fixture and stored), which holds at most 0.1 % of
the tokens (else: another seed); the numpy float64 orthogonal loss and gradient equal torch's float64 ones.

    python tools/gen_golden_lucid.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import oracle, refimport  # noqa: E402
from dynamicvectorquantization_amd import synth  # noqa: E402
from tests import _lucid_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
G_SEEN = [0.0]
SIDE_BYTES = 96 << 10


def classes():
    refimport.setup()
    import modules.vector_quantization.quantize_lucidrains as ql
    return ql


def save(name, rec):
    for f in os.listdir(OUT):
        if f.startswith("lucid_%s." % name):
            os.remove(os.path.join(OUT, f))
    for field in list(rec):
        arr = rec[field]
        if isinstance(arr, np.ndarray) and arr.nbytes > SIDE_BYTES:       # a side file of its own, in parts of at most PART_BYTES
            n_rows = max(1, R.PART_BYTES // (arr.nbytes // arr.shape[0]))
            parts = [arr[i:i + n_rows] for i in range(0, arr.shape[0], n_rows)]
            for i, part in enumerate(parts):
                np.savez_compressed(os.path.join(OUT, "lucid_%s.%s%d.npz" % (name, field, i)), a=part)
            rec[field + "_parts"] = np.int64(len(parts))
            del rec[field]
    np.savez_compressed(os.path.join(OUT, "lucid_%s.npz" % name), **rec)
    sizes = [os.path.getsize(os.path.join(OUT, f)) for f in os.listdir(OUT) if f.startswith("lucid_%s." % name)]
    assert max(sizes) <= R.PART_BYTES + (16 << 10), sizes
    return sizes


def rows_t(x, layout):
    return torch.from_numpy(R.rows_of(x.numpy(), layout))


def picks_for(seed, N, K):
    """K distinct token indices when the batch has them, K indices otherwise"""
    order = np.argsort(synth.uniform(seed, (N,)), kind="stable").astype(np.int64)
    return order[:K] if N >= K else np.concatenate([order, synth.randint(seed + 1, (K - N,), N)])


def build(ql, cosine, K, D, kw, E, embed_avg, cs0, picks, temp):
    m = ql.VectorQuantize(K, D, sample_codebook_temp=temp, sync_codebook=False, **kw)
    if cosine:
        ckw = dict(dim=D, codebook_size=K, decay=kw.get("decay", 0.8), threshold_ema_dead_code=kw.get("threshold_ema_dead_code", 0),
                   learnable_codebook=kw.get("orthogonal_reg_weight", 0.) > 0, sample_codebook_temp=temp)
        m._codebook = ql.CosineSimCodebook(**ckw)
    cb = m._codebook
    with torch.no_grad():
        cb.embed.copy_(torch.from_numpy(E).unsqueeze(0))
        if not cosine:
            cb.embed_avg.copy_(torch.from_numpy(embed_avg).unsqueeze(0))
        cb.cluster_size.copy_(torch.from_numpy(cs0).unsqueeze(0))
    pk = torch.from_numpy(picks)
    cb.sample_fn = lambda samples, num: samples[:, pk[:num]]
    return m


def fixture(tag, cosine, kw, layout, E, embed_avg, cs0, x, temp1, seed, train=True):
    ql = classes()
    K, D = E.shape
    xt = torch.from_numpy(x)
    rows = rows_t(xt, layout)
    N = rows.shape[0]
    picks = picks_for(seed + 500, N, K)
    gq = synth.normal(seed + 600, x.shape, 0.0, 1e-3)
    cw = float(kw.get("commitment_weight", 1.0))
    ow = float(kw.get("orthogonal_reg_weight", 0.0))
    rec = dict(cosine=np.array(bool(cosine)), layout=np.array(layout), D=np.int64(D), K=np.int64(K), E=E, x=x, cs0=cs0, picks=picks,
               gq=gq, decay=np.float64(kw.get("decay", 0.8)), eps=np.float64(1e-5),
               threshold=np.float64(kw.get("threshold_ema_dead_code", 0)), commitment_weight=np.float64(cw),
               orthogonal_reg_weight=np.float64(ow), seed=np.int64(seed))
    if not cosine:
        rec["embed_avg"] = embed_avg
    m0 = build(ql, cosine, K, D, kw, E, embed_avg, cs0, picks, 0.)
    rec["state_keys"] = np.array(sorted(m0.state_dict().keys()))
    rec["state_shapes"] = np.array([",".join(str(s) for s in m0.state_dict()[k].shape) for k in sorted(m0.state_dict().keys())])

    # scores: the reference's own fp32 `dist`, the float64 value, the kernels' -sqrt(oracle d) (cosine: the dot products)
    Et = torch.from_numpy(E)
    if cosine:
        a, b = torch.nn.functional.normalize(rows, p=2, dim=-1), torch.nn.functional.normalize(Et, p=2, dim=-1)
        dist32 = (a @ b.t()).numpy()
        dist64 = (a.double() @ b.double().t()).numpy()
        score = dist32                                   # the restatement's scores: the reference's normalised operands' dots
        rec.update(xn=a.numpy(), wn=b.numpy())
    else:
        dist32 = (-torch.cdist(rows.unsqueeze(0), Et.unsqueeze(0), p=2))[0].numpy()
        dist64 = (-torch.cdist(rows.double().unsqueeze(0), Et.double().unsqueeze(0), p=2))[0].numpy()
        od = np.stack([oracle.token_distances(rows[n].numpy(), E) for n in range(N)]).astype(np.float32)
        score = R.cdist_scores(od)
        rec["d"] = od
    fin = np.isfinite(dist64).all(axis=1)
    s_err = max(float(np.abs(dist32[fin].astype(np.float64) - dist64[fin]).max()),
                float(np.abs(score[fin].astype(np.float64) - dist64[fin]).max()))
    rec["S_ERR"] = np.float64(s_err)

    def run(m, training, seed_):
        m.train(training)
        xin = xt.clone().requires_grad_(training)
        if seed_ is not None:
            torch.manual_seed(seed_)
        q, loss, (_, _, ind) = m(xin)
        out = dict(codes=ind.numpy().copy(), loss=np.float32(loss.detach().item()))
        codes = ind.reshape(-1)
        e_rows = Et[codes]
        if layout == "nchw":
            e_img = e_rows.reshape(x.shape[0], -1, D).permute(0, 2, 1).reshape(x.shape)
        else:
            e_img = e_rows.reshape(x.shape)
        with torch.no_grad():
            want = (xt + (e_img - xt)) if training else e_img
        assert np.array_equal(q.detach().numpy().view(np.uint32), want.numpy().view(np.uint32)), \
            "%s: quantize is not %s" % (tag, "fl(x + fl(e - x))" if training else "embed[codes]")
        if training:
            (loss.sum() + (q * torch.from_numpy(gq)).sum()).backward()
            out["xgrad"] = xin.grad.numpy().copy()
            cb = m._codebook
            out["embed_after"] = cb.embed.detach()[0].numpy().copy()
            out["cs_after"] = cb.cluster_size[0].numpy().copy()
            if not cosine:
                assert np.array_equal(cb.embed_avg[0].numpy(), embed_avg), "%s: embed_avg changed" % tag
            if ow > 0:
                out["embed_grad"] = cb.embed.grad[0].numpy().copy()
                l64, g64 = R.ortho64(out["embed_after"])
                out["embed_grad_err32"] = np.float64(np.abs(out["embed_grad"].astype(np.float64) - ow * g64).max()
                                                     / np.abs(ow * g64).max())
        return out

    # temp 0: eval, then a training step of a fresh module
    ev = run(build(ql, cosine, K, D, kw, E, embed_avg, cs0, picks, 0.), False, None)
    hard = R.argmax_torch(score) if cosine else R.argmin_torch(rec["d"])
    assert np.array_equal(hard, ev["codes"].reshape(-1)), "%s: the restatement's hard codes are not the reference's" % tag
    rec.update(codes_eval0=ev["codes"], loss_eval0=ev["loss"])
    if train:
        tr = run(build(ql, cosine, K, D, kw, E, embed_avg, cs0, picks, 0.), True, None)
        assert np.array_equal(tr["codes"], ev["codes"])
        rec.update({k + "_train0": v for k, v in tr.items()})
    share = 0.0
    if temp1 is not None:
        for attempt in range(20):
            s1 = seed + attempt
            tr = run(build(ql, cosine, K, D, kw, E, embed_avg, cs0, picks, temp1), train, s1)
            torch.manual_seed(s1)
            u = torch.zeros(1, N, K).uniform_(0, 1)[0].numpy()
            g32 = -torch.log((-torch.log(torch.from_numpy(u).clamp(min=1e-20))).clamp(min=1e-20)).numpy()
            again = R.argmax_torch((dist32 / np.float32(temp1)) + g32)
            assert np.array_equal(again, tr["codes"].reshape(-1)), "%s: replayed u is not the forward's noise" % tag
            G_SEEN[0] = max(G_SEEN[0], float(np.abs(g32.astype(np.float64) - R.gumbel64(u)).max()))
            skip = R.skip_sampled(score, temp1, u, s_err)
            mine = R.argmax_torch(R.perturbed(score, temp1, u))
            share = float(skip.mean())
            if share <= R.SKIP_CAP and np.array_equal(mine[~skip], tr["codes"].reshape(-1)[~skip]):
                break
        else:
            raise AssertionError("%s: no seed keeps the skip set under the cap" % tag)
        sfx = "_train1" if train else "_eval1"
        rec.update({k + sfx: v for k, v in tr.items()})
        rec.update(temp1=np.float32(temp1), seed1=np.int64(s1), u1=u, skip1=skip)
    sizes = save(tag, rec)
    print("%s: N %d  S_ERR %.3g  skip share %.5f  files %d, largest %d bytes" % (tag, N, s_err, share, len(sizes), max(sizes)))


def cosine_direct(tag, E, cs0, x, seed):
    """CosineSimCodebook called directly: eval and a training step with expiry"""
    ql = classes()
    K, D = E.shape
    N = x.reshape(-1, D).shape[0]
    picks = picks_for(seed + 500, N, K)
    pk = torch.from_numpy(picks)
    rec = dict(D=np.int64(D), K=np.int64(K), E=E, x=x, cs0=cs0, picks=picks, decay=np.float64(0.8), threshold=np.float64(2))

    def make():
        cb = ql.CosineSimCodebook(D, K, decay=0.8, threshold_ema_dead_code=2)
        with torch.no_grad():
            cb.embed.copy_(torch.from_numpy(E).unsqueeze(0))
            cb.cluster_size.copy_(torch.from_numpy(cs0).unsqueeze(0))
        cb.sample_fn = lambda samples, num: samples[:, pk[:num]]
        return cb

    cb = make().eval()
    q, ind = cb(torch.from_numpy(x))
    assert np.array_equal(q.numpy(), E[ind.numpy()])
    rec.update(codes_eval=ind.numpy().copy(), state_keys=np.array(sorted(cb.state_dict().keys())))
    cb = make().train()
    q, ind = cb(torch.from_numpy(x))
    assert np.array_equal(q.numpy(), E[ind.numpy()]) and np.array_equal(ind.numpy(), rec["codes_eval"])
    rec.update(embed_after=cb.embed[0].numpy().copy(), cs_after=cb.cluster_size[0].numpy().copy())
    new, cs, expired = R.train_step(1, x.reshape(-1, D), ind.numpy(), E, None, cs0, 0.8, 1e-5, 2.0, picks)
    assert expired.any() and not expired.all()
    assert np.abs(new - rec["embed_after"]).max() <= 1e-5 * np.abs(new).max()
    sizes = save(tag, rec)
    print("%s: N %d  expired %d  largest %d bytes" % (tag, N, int(expired.sum()), max(sizes)))


def tie_case():
    E = synth.codebook_trained(96, 64, seed=9141).copy()
    E[70], E[33], E[95] = E[5], E[12], E[40]
    x = np.ascontiguousarray(synth.z_tokens(E, 1, 40, 1, 9142)[0, :, :, 0].T)
    x[0], x[1], x[4] = E[70], E[33], E[95]          # equal to a duplicated code: the first of the pair wins
    x[2, 17] = np.nan                               # every score NaN: the first NaN, index 0
    x[3] = 0.0                                      # the zero token
    x[5] = 2.0 * E[70]
    return E, x.reshape(1, 40, 64)


def ortho_set(name, t):
    ql = classes()
    t32 = torch.from_numpy(t).unsqueeze(0).requires_grad_(True)
    l32 = ql.orthogonal_loss_fn(t32)
    l32.backward()
    t64 = torch.from_numpy(t).double().unsqueeze(0).requires_grad_(True)
    l64 = ql.orthogonal_loss_fn(t64)
    l64.backward()
    mine_l, mine_g = R.ortho64(t)
    g64 = t64.grad[0].numpy()
    assert abs(mine_l - float(l64)) <= 1e-12 * abs(float(l64)) and np.abs(mine_g - g64).max() <= 1e-12 * np.abs(g64).max(), name
    err32 = float(np.abs(t32.grad[0].numpy().astype(np.float64) - g64).max() / np.abs(g64).max())
    sizes = save("e_ortho_" + name, dict(t=t, loss32=np.float32(l32.item()), loss64=np.float64(l64.item()), grad_err32=np.float64(err32)))
    print("e_ortho_%s: loss %.8g (fp32 %.8g)  fp32 gradient error %.3g  %d bytes" % (name, float(l64), float(l32), err32, max(sizes)))


def kmeans_fixture():
    ql = classes()
    K, D, N = 64, 64, 512
    E = synth.codebook_trained(K, D, seed=9161)
    x = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, 9162)[0, :, :, 0].T).reshape(1, N, D)
    init = picks_for(9163, N, K)
    rec = dict(x=x, init=init, K=np.int64(K), D=np.int64(D), iters=np.int64(3))
    for cosine in (False, True):
        m = ql.VectorQuantize(K, D, kmeans_init=True, kmeans_iters=3, sync_codebook=False)
        if cosine:
            m._codebook = ql.CosineSimCodebook(D, K, kmeans_init=True, kmeans_iters=3, threshold_ema_dead_code=0)
        it = torch.from_numpy(init)
        m._codebook.sample_fn = lambda samples, num: samples[:, it[:num]]
        m.eval()
        with torch.no_grad():
            _, _, (_, _, ind) = m(torch.from_numpy(x))
        assert float(m._codebook.initted) == 1.0
        sfx = "_cos" if cosine else ""
        rec.update({"means" + sfx: m._codebook.embed[0].numpy().copy(), "bins" + sfx: m._codebook.cluster_size[0].numpy().copy(),
                    "codes" + sfx: ind.numpy().copy()})
    sizes = save("f_kmeans", rec)
    print("f_kmeans: largest %d bytes" % max(sizes))


def main():
    E = synth.codebook_trained(96, 256, seed=9101)
    fixture("a_euclid", False, dict(decay=0.8, threshold_ema_dead_code=2, accept_image_fmap=True, orthogonal_reg_weight=0.5), "nchw",
            E, synth.codebook_trained(96, 256, seed=9104), synth.uniform(9105, (96,), 0.0, 12.0),
            synth.z_tokens(E, 2, 8, 8, 9102), 1.0, 91)
    E = synth.codebook_trained(1024, 64, seed=9111)
    x = np.ascontiguousarray(synth.z_tokens(E, 1, 200, 1, 9112)[0, :, :, 0].T).reshape(1, 200, 64)
    fixture("b_euclid_flat", False, dict(decay=0.8), "flat", E, synth.codebook_trained(1024, 64, seed=9114),
            synth.uniform(9115, (1024,), 0.0, 4.0), x, 0.5, 92)
    E = synth.codebook_trained(160, 128, seed=9121)
    x = np.ascontiguousarray(synth.z_tokens(E, 2, 63, 1, 9122)[:, :, :, 0].transpose(0, 2, 1))
    cs0 = synth.uniform(9125, (160,), 0.0, 12.0)
    fixture("c_cosine", True, dict(decay=0.8, threshold_ema_dead_code=2), "flat", E, None, cs0, x, None, 93)
    cosine_direct("c_cosine_direct", E, cs0, x, 93)
    E, x = tie_case()
    fixture("d_ties", False, dict(), "flat", E, E.copy(), np.zeros(96, np.float32), x, None, 94, train=False)
    for n, d, s in ((96, 64, 9131), (100, 256, 9133), (1024, 128, 9135)):
        ortho_set("n%d_d%d_init" % (n, d), synth.codebook_default_init(n, d, seed=s))
        ortho_set("n%d_d%d_trained" % (n, d), synth.codebook_trained(n, d, seed=s + 1))
    t = synth.codebook_trained(96, 64, seed=9139).copy()
    t[40], t[77] = t[3], t[3]
    t[11] = 0.0
    ortho_set("n96_d64_dup_zero", t)
    kmeans_fixture()
    print("largest |g32 - g64| over the stored u: %r  (tests/_maskvq_ref.py: G_ERR = %r)" % (G_SEEN[0], R.G_ERR))
    assert G_SEEN[0] <= R.G_ERR, "the gumbel noise of a stored u exceeds G_ERR of tests/_maskvq_ref.py"


if __name__ == "__main__":
    main()
