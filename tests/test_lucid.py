"""The lucidrains-style quantizer (dynamicvectorquantization_amd/lucid.py): EuclideanCodebook, CosineSimCodebook, VectorQuantize,
orthogonal_loss_fn, the cdist-sampled assign (dvq_vq_cdist_sample_assign_f32), the fused orthogonal loss
(dvq_ortho_loss_*_f32) and the codebook update (dvq_lucid_update_f32), against the reference's own classes on the CPU
(tests/golden/lucid_*.npz, written by tools/gen_golden_lucid.py) and the numpy restatement tests/_lucid_ref.py, whose docstring
derives the skip rule of the sampled codes.

Tolerances.  cluster_size: 1e-5 relative per element.  embed after a step: 1e-5 of the largest |reference| element (the cosine
update is a sum of two terms that may cancel in an element; the Euclidean one is a quotient, and meets the bound per element too).
After a training step the GPU's state is compared with the float64 restatement run on the GPU's OWN codes (the restatement is
pinned to the reference by the CPU tests), so a sampled code inside the skip set does not fail the comparison of what follows."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _lucid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIX = {}
NEW = ("dvq_vq_cdist_sample_assign_f32", "dvq_ortho_loss_workspace_bytes", "dvq_ortho_loss_forward_f32",
       "dvq_ortho_loss_backward_f32", "dvq_lucid_update_f32")
TRAINED = ("a_euclid", "b_euclid_flat", "c_cosine")


def _fixture(tag):
    """loaded once and shared read-only"""
    if tag not in _FIX:
        g = R.load(tag)
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FIX[tag] = g
    return _FIX[tag]


def _variants(g):
    """[(suffix, temp, u or None)] of the fixture's training steps"""
    out = [("0", 0.0, None)]
    if "temp1" in g:
        out.append(("1", float(g["temp1"]), g["u1"]))
    return out


def _scores(g):
    return g["xn"] @ g["wn"].T if bool(g["cosine"]) else R.cdist_scores(g["d"])


def _kw(g):
    kw = dict(decay=float(g["decay"]), threshold_ema_dead_code=float(g["threshold"]), use_cosine_sim=bool(g["cosine"]),
              orthogonal_reg_weight=float(g["orthogonal_reg_weight"]), commitment_weight=float(g["commitment_weight"]))
    if str(g["layout"]) == "nchw":
        kw["accept_image_fmap"] = True
    return kw


def _e_img(g, codes):
    """embed[codes] in the layout of the module input"""
    x, E = g["x"], g["E"]
    e = E[codes.reshape(-1)]
    if str(g["layout"]) == "nchw":
        return np.ascontiguousarray(e.reshape(x.shape[0], -1, x.shape[1]).transpose(0, 2, 1)).reshape(x.shape)
    return e.reshape(x.shape)


def _expected_step(g, codes):
    """the float64 restatement's (embed', cluster_size', expired, loss, x.grad) of a training step that chose `codes`"""
    rows = R.rows_of(g["x"], str(g["layout"]))
    kind = 1 if bool(g["cosine"]) else 0
    new, cs, expired = R.train_step(kind, rows, codes, g["E"], g.get("embed_avg"), g["cs0"], float(g["decay"]), float(g["eps"]),
                                    float(g["threshold"]), g["picks"])
    cw, ow = float(g["commitment_weight"]), float(g["orthogonal_reg_weight"])
    e = g["E"][codes.reshape(-1)]
    loss = R.commit_loss(rows, e, cw)
    if ow > 0:
        loss += ow * R.ortho64(new.astype(np.float32))[0]
    xgrad = g["gq"].astype(np.float64) + cw * 2.0 * (g["x"].astype(np.float64) - _e_img(g, codes)) / g["x"].size
    return new, cs, expired, loss, xgrad


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_declared_and_exported():
    from dynamicvectorquantization_amd import _lib, lucid  # noqa: F401
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvq.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.EXPORTS
    assert _lib.lib.dvq_version() >= 1600


def test_abi_validation_without_gpu():
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    a = 256                                                        # a "pointer" that passes the alignment checks

    def cd(x=a, prep=a, B=2, D=256, HW=64, K=96, temp=1.0, u=a, un=128 * 96, codes=a):
        return L.dvq_vq_cdist_sample_assign_f32(x, prep, B, D, HW, K, temp, u, un, codes, 0)

    for null in ("x", "prep", "codes", "u"):
        assert cd(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert cd(un=128 * 96 - 1) == EINVAL and b"u has" in L.dvq_last_error_string()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert cd(temp=bad) == EINVAL and b"temp" in L.dvq_last_error_string()
    assert cd(B=0) == EINVAL and cd(K=0) == EINVAL
    assert cd(x=a + 2) == EINVAL and cd(prep=a + 16) == EINVAL
    assert cd(D=100) == EUNSUPPORTED and b"zero channels" in L.dvq_last_error_string()

    assert L.dvq_ortho_loss_workspace_bytes(1, 96, 100) == 0 and L.dvq_ortho_loss_workspace_bytes(0, 96, 64) == 0
    need = L.dvq_ortho_loss_workspace_bytes(1, 1024, 128)
    assert need >= 8 * 1024 * 128 * 4 and need % 256 == 0         # 8 column slices of partial gradients (forward: 32 doubles)

    def of(t=a, h=1, n=1024, d=128, rinv=a, loss=a, ws=a, wsb=need):
        return L.dvq_ortho_loss_forward_f32(t, h, n, d, rinv, loss, ws, wsb, 0)

    for null in ("t", "rinv", "loss"):
        assert of(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert of(n=0) == EINVAL and of(h=0) == EINVAL
    assert of(d=96) == EUNSUPPORTED and of(d=512) == EUNSUPPORTED
    assert of(wsb=need - 1) == EWORKSPACE and of(ws=0) == EWORKSPACE
    assert of(t=a + 4) == EINVAL and of(ws=a + 64) == EINVAL

    nb = L.dvq_ortho_loss_workspace_bytes(1, 96, 64)
    assert nb >= 3 * 96 * 64 * 4                                   # the backward's three column slices of partial gradients

    def ob(t=a, rinv=a, g=a, h=1, n=96, d=64, grad=2 * a, ws=a, wsb=nb):
        return L.dvq_ortho_loss_backward_f32(t, rinv, g, h, n, d, grad, ws, wsb, 0)

    for null in ("t", "rinv", "g", "grad"):
        assert ob(**{null: 0}) == EINVAL
    assert ob(grad=a) == EINVAL and b"alias" in L.dvq_last_error_string()
    assert ob(n=0) == EINVAL and ob(d=100) == EUNSUPPORTED
    assert ob(wsb=nb - 1) == EWORKSPACE and ob(ws=0) == EWORKSPACE and ob(ws=a + 64) == EINVAL

    def up(kind=0, counts=a, sums=0, decay=0.8, eps=1e-5, thr=2.0, K=96, D=64, cs=a, cso=2 * a, avg=3 * a, embed=4 * a, x=a, B=2,
           HW=64, pick=a):
        return L.dvq_lucid_update_f32(kind, counts, sums, decay, eps, thr, K, D, cs, cso, avg, embed, x, B, HW, pick, 0)

    assert up(kind=2) == EINVAL and b"kind" in L.dvq_last_error_string()
    for null in ("counts", "cs", "cso", "embed", "avg"):
        assert up(**{null: 0}) == EINVAL
    assert up(kind=1, sums=0) == EINVAL and b"sums" in L.dvq_last_error_string()
    assert up(cso=a) == EINVAL and b"alias" in L.dvq_last_error_string()
    assert up(embed=3 * a) == EINVAL
    assert up(K=0) == EINVAL and up(D=0) == EINVAL
    assert up(decay=1.5) == EINVAL and up(thr=-1.0) == EINVAL
    assert up(x=0) == EINVAL and up(HW=0) == EINVAL               # expiry (pick given) needs the batch


@pytest.mark.parametrize("tag", R.FIXTURES)
def test_restatement_reproduces_the_reference(tag):
    """tests/_lucid_ref.py gives the reference's hard codes from the assign's distances (cosine: from the reference's operands),
    its sampled codes outside the skip set -- which stays under the cap -- and, from the reference's codes, its embed,
    cluster_size and loss after a training step"""
    g = _fixture(tag)
    s = _scores(g)
    hard = R.argmax_torch(s) if bool(g["cosine"]) else R.argmin_torch(g["d"])
    assert np.array_equal(hard, g["codes_eval0"].reshape(-1))
    assert float(g["loss_eval0"]) == 0.0
    if "temp1" in g:
        temp, u = float(g["temp1"]), g["u1"]
        skip = R.skip_sampled(s, temp, u, float(g["S_ERR"]))
        assert np.array_equal(skip, g["skip1"]) and skip.mean() <= R.SKIP_CAP
        mine = R.argmax_torch(R.perturbed(s, temp, u))
        assert np.array_equal(mine[~skip], g["codes_train1"].reshape(-1)[~skip])
    if tag not in TRAINED:
        return
    for sfx, _, _ in _variants(g):
        codes = g["codes_train" + sfx]
        new, cs, expired, loss, xgrad = _expected_step(g, codes)
        assert np.abs(cs - g["cs_after_train" + sfx]).max() <= 1e-5 * np.abs(cs).max()
        assert np.abs(new - g["embed_after_train" + sfx]).max() <= 1e-5 * np.abs(new).max()
        assert abs(loss - float(g["loss_train" + sfx])) <= 1e-5 * abs(loss)
        assert np.abs(xgrad - g["xgrad_train" + sfx]).max() <= 1e-6
        if float(g["threshold"]) > 0:
            assert expired.any() and not expired.all()
            assert np.abs(np.linalg.norm(g["embed_after_train" + sfx][expired].astype(np.float64), axis=1) - 1.0).max() <= 1e-6


def test_state_dict_parameters_and_refusals():
    from dynamicvectorquantization_amd import _lib, lucid
    for tag in ("a_euclid", "c_cosine"):
        g = _fixture(tag)
        m = lucid.VectorQuantize(int(g["K"]), int(g["D"]), **_kw(g))
        sd = m.state_dict()
        assert sorted(sd.keys()) == list(g["state_keys"])
        assert [",".join(str(s) for s in sd[k].shape) for k in sorted(sd.keys())] == list(g["state_shapes"])
        assert isinstance(m._codebook, lucid.CosineSimCodebook if bool(g["cosine"]) else lucid.EuclideanCodebook)
        assert tuple(m.codebook.shape) == (int(g["K"]), int(g["D"]))
    assert sorted(lucid.CosineSimCodebook(128, 160).state_dict().keys()) == list(_fixture("c_cosine_direct")["state_keys"])
    for ow in (0.0, 0.5):
        for cos in (False, True):
            m = lucid.VectorQuantize(32, 64, orthogonal_reg_weight=ow, use_cosine_sim=cos)
            assert isinstance(m._codebook.embed, torch.nn.Parameter) == (ow > 0)
            assert ("_codebook.embed" in dict(m.named_parameters())) == (ow > 0)
    assert lucid.VectorQuantize(32, 64, orthogonal_reg_max_codes=8).orthogonal_reg_max_codes == 8    # accepted, inert
    with pytest.raises(NotImplementedError, match="IndexError"):
        lucid.VectorQuantize(32, 64, orthogonal_reg_weight=0.5, orthogonal_reg_active_codes_only=True)
    m = lucid.VectorQuantize(32, 64)
    with pytest.raises(_lib.DvqError):
        m(torch.zeros(1, 5, 64))
    with pytest.raises(_lib.DvqError):
        lucid.EuclideanCodebook(64, 32)(torch.zeros(1, 5, 64))
    k = lucid.VectorQuantize(8, 64, kmeans_init=True)
    assert float(k._codebook.initted) == 0.0 and float(k._codebook.embed.abs().max()) == 0.0
    # default init: the cosine codebook's rows have norm 1
    assert np.abs(lucid.CosineSimCodebook(64, 32).embed[0].norm(dim=-1).numpy() - 1.0).max() <= 1e-6


def test_orthogonal_loss_cpu_is_the_reference_expression():
    from dynamicvectorquantization_amd import lucid
    g = _fixture("e_ortho_n96_d64_dup_zero")
    t = torch.tensor(g["t"], dtype=torch.float64, requires_grad=True)
    loss = lucid.orthogonal_loss_fn(t)                             # [n, d]: h = 1
    loss.backward()
    loss = loss.detach()
    l64, g64 = R.ortho64(g["t"])
    assert abs(float(loss) - float(g["loss64"])) <= 1e-12 * float(g["loss64"]) and abs(l64 - float(g["loss64"])) <= 1e-12 * l64
    assert np.abs(t.grad.numpy() - g64).max() <= 1e-12 * np.abs(g64).max()
    assert abs(float(lucid.orthogonal_loss_fn(torch.tensor(g["t"]).unsqueeze(0))) - float(g["loss32"])) <= 1e-6 * float(g["loss32"])


def test_new_class_takes_the_generic_encode_path():
    from dynamicvectorquantization_amd import encode, lucid
    h = torch.zeros(1, 256, 4, 4)
    conv = torch.nn.Conv2d(256, 256, 1)
    m = lucid.VectorQuantize(96, 256, accept_image_fmap=True).eval()
    assert encode._can_route(m, None, h, h) is False
    assert encode._can_route_conv(m, conv, h, h) is False
    assert encode._can_fold(m, conv, h, h) is False
    assert encode._can_fuse_vqgan(m, conv, h) is False


# ---------------------------------------------------------------------------------------------------------------- GPU

def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _module(g, dev, temp=0.0):
    from dynamicvectorquantization_amd import lucid
    m = lucid.VectorQuantize(int(g["K"]), int(g["D"]), sample_codebook_temp=temp, **_kw(g)).to(dev)
    cb = m._codebook
    with torch.no_grad():
        cb.embed.copy_(_t(g["E"], dev).unsqueeze(0))
        if not bool(g["cosine"]):
            cb.embed_avg.copy_(_t(g["embed_avg"], dev).unsqueeze(0))
        cb.cluster_size.copy_(_t(g["cs0"], dev).unsqueeze(0))
    cb.invalidate_codebook_cache()
    cb._expire_pick = _t(g["picks"], dev)
    return m


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", R.FIXTURES)
def test_eval_codes_and_quantize(tag, dev):
    """temp 0: every code is the reference's (d_ties: duplicated rows, a NaN token, a zero token), quantize = embed[codes] bit for
    bit, loss = [0.]"""
    g = _fixture(tag)
    m = _module(g, dev).eval()
    with torch.no_grad():
        q, loss, (a, b, ind) = m(_t(g["x"], dev))
    assert a is None and b is None and ind.dtype == torch.int64
    codes = ind.cpu().numpy()
    assert codes.shape == g["codes_eval0"].shape and np.array_equal(codes, g["codes_eval0"])
    assert np.array_equal(_bits(q.cpu().numpy()), _bits(_e_img(g, codes)))
    assert tuple(loss.shape) == (1,) and float(loss) == 0.0 and not loss.requires_grad
    ent = m.get_codebook_entry(ind.reshape(ind.shape[0], -1))
    assert np.array_equal(_bits(ent.cpu().numpy()), _bits(g["E"][codes.reshape(codes.shape[0], -1)]))


@pytest.mark.gpu
@pytest.mark.parametrize("tag,sfx", [(t, s) for t in TRAINED for s in ("0", "1") if not (t == "c_cosine" and s == "1")])
def test_training_step(tag, sfx, dev, monkeypatch):
    from dynamicvectorquantization_amd import lucid
    g = _fixture(tag)
    temp = 0.0 if sfx == "0" else float(g["temp1"])
    if sfx == "1":
        u = _t(g["u1"], dev)
        monkeypatch.setattr(lucid, "_draw_uniform", lambda N, K, device: u)
    m = _module(g, dev, temp).train()
    cb = m._codebook
    avg0 = None if bool(g["cosine"]) else cb.embed_avg.detach().clone()
    x = _t(g["x"], dev).requires_grad_(True)
    q, loss, (_, _, ind) = m(x)
    (loss.sum() + (q * _t(g["gq"], dev)).sum()).backward()
    loss = loss.detach()
    codes = ind.cpu().numpy()
    ref = g["codes_train" + sfx]
    assert codes.shape == ref.shape
    if sfx == "0":
        assert np.array_equal(codes, ref)
    else:
        skip = R.skip_sampled(_scores(g), temp, g["u1"], float(g["S_ERR"]))
        assert skip.mean() <= R.SKIP_CAP
        assert np.array_equal(codes.reshape(-1)[~skip], ref.reshape(-1)[~skip])
    # quantize = fl(x + fl(e - x)) of the rows BEFORE the update, bit for bit
    e = _e_img(g, codes)
    assert np.array_equal(_bits(q.detach().cpu().numpy()), _bits(g["x"] + (e - g["x"])))
    new, cs, expired, want_loss, want_xgrad = _expected_step(g, codes)
    print("%s%s: loss %.9g (restated %.9g, reference %.9g)" % (tag, sfx, float(loss), want_loss, float(g["loss_train" + sfx])))
    assert tuple(loss.shape) == (1,) and abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss)
    assert np.abs(x.grad.cpu().numpy() - want_xgrad).max() <= 1e-6
    got_cs, got_e = cb.cluster_size[0].cpu().numpy(), cb.embed.detach()[0].cpu().numpy()
    assert np.abs(got_cs - cs).max() <= 1e-5 * np.abs(cs).max() and np.all(np.abs(got_cs - cs) <= 1e-5 * np.abs(cs) + 1e-30)
    assert np.abs(got_e - new).max() <= 1e-5 * np.abs(new).max()
    if not bool(g["cosine"]):
        assert torch.equal(cb.embed_avg, avg0)                     # never written
        assert np.all(np.abs(got_e - new)[~expired] <= 1e-5 * np.abs(new)[~expired] + 1e-30)
    if np.array_equal(codes, ref):                                  # the same codes: the reference's own numbers
        assert abs(float(loss) - float(g["loss_train" + sfx])) <= 1e-5 * abs(float(g["loss_train" + sfx]))
        assert np.abs(x.grad.cpu().numpy() - g["xgrad_train" + sfx]).max() <= 1e-6
        assert np.abs(got_cs - g["cs_after_train" + sfx]).max() <= 1e-5 * np.abs(cs).max()
        assert np.abs(got_e - g["embed_after_train" + sfx]).max() <= 1e-5 * np.abs(new).max()
    if float(g["threshold"]) > 0:
        rows = R.l2norm(R.rows_of(g["x"], str(g["layout"])).astype(np.float64))
        assert expired.any() and np.abs(got_e[expired] - rows[g["picks"][:int(expired.sum())]]).max() <= 1e-6
    if float(g["orthogonal_reg_weight"]) > 0:
        # embed.grad = ow * d ortho / d embed at the UPDATED embed: the fp32-gradient rule of test_orthogonal_loss
        ow = float(g["orthogonal_reg_weight"])
        g64 = ow * R.ortho64(got_e)[1]
        err = np.abs(cb.embed.grad[0].cpu().numpy() - g64).max() / np.abs(g64).max()
        print("%s%s: embed.grad error %.3g, the reference's fp32 %.3g" % (tag, sfx, err, float(g["embed_grad_err32_train" + sfx])))
        assert err <= 4.0 * float(g["embed_grad_err32_train" + sfx])


@pytest.mark.gpu
def test_cosine_codebook_direct(dev):
    from dynamicvectorquantization_amd import lucid
    g = _fixture("c_cosine_direct")
    K, D = int(g["K"]), int(g["D"])
    cb = lucid.CosineSimCodebook(D, K, decay=0.8, threshold_ema_dead_code=2).to(dev)
    with torch.no_grad():
        cb.embed.copy_(_t(g["E"], dev).unsqueeze(0))
        cb.cluster_size.copy_(_t(g["cs0"], dev).unsqueeze(0))
    cb._expire_pick = _t(g["picks"], dev)
    cb.eval()
    q, ind = cb(_t(g["x"], dev))
    assert np.array_equal(ind.cpu().numpy(), g["codes_eval"]) and np.array_equal(_bits(q.cpu().numpy()), _bits(g["E"][g["codes_eval"]]))
    cb.train()
    q, ind = cb(_t(g["x"], dev))
    assert np.array_equal(ind.cpu().numpy(), g["codes_eval"]) and np.array_equal(_bits(q.cpu().numpy()), _bits(g["E"][g["codes_eval"]]))
    assert np.abs(cb.cluster_size[0].cpu().numpy() - g["cs_after"]).max() <= 1e-5 * np.abs(g["cs_after"]).max()
    assert np.abs(cb.embed[0].cpu().numpy() - g["embed_after"]).max() <= 1e-5 * np.abs(g["embed_after"]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name", R.ORTHO_SETS)
def test_orthogonal_loss(name, dev):
    """value within 1e-5 relative of the float64 one; two calls bit-identical; the gradient's max-abs error against the float64
    gradient, normalised by max |g64|, at most 4 x that of the reference's own fp32 CPU gradient (the factor: the two sides sum
    n terms in different orders)"""
    from dynamicvectorquantization_amd import lucid
    g = _fixture("e_ortho_" + name)
    _, g64 = R.ortho64(g["t"])
    runs = []
    for _ in range(2):
        t = _t(g["t"], dev).unsqueeze(0).requires_grad_(True)
        loss = lucid.orthogonal_loss_fn(t)
        assert type(loss.grad_fn).__name__.startswith("_OrthogonalLoss")          # the kernels, not the torch expression
        (loss * 1.5).backward()
        runs.append((loss.detach().cpu().numpy().copy(), t.grad[0].cpu().numpy().copy()))
    assert np.array_equal(_bits(runs[0][0].reshape(1)), _bits(runs[1][0].reshape(1))) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))
    val, grad = float(runs[0][0]), runs[0][1]
    err = np.abs(grad.astype(np.float64) - 1.5 * g64).max() / np.abs(1.5 * g64).max()
    print("%s: loss %.9g (float64 %.9g)  gradient error %.3g, the reference's fp32 %.3g" % (name, val, float(g["loss64"]), err, float(g["grad_err32"])))
    assert abs(val - float(g["loss64"])) <= 1e-5 * float(g["loss64"])
    assert np.isfinite(grad).all() and err <= 4.0 * float(g["grad_err32"])
    two = lucid.orthogonal_loss_fn(_t(g["t"], dev))                # [n, d]: h = 1
    assert np.array_equal(_bits(two.cpu().numpy().reshape(1)), _bits(runs[0][0].reshape(1)))


@pytest.mark.gpu
@pytest.mark.parametrize("cosine", [False, True])
def test_kmeans_init(cosine, dev):
    """the reference's k-means from the same initial rows: means within rounding (the tolerance of test_maskvq's test_kmeans_init),
    `initted` set, cluster_size = the last bins"""
    from dynamicvectorquantization_amd import lucid
    g = _fixture("f_kmeans")
    K, D = int(g["K"]), int(g["D"])
    sfx = "_cos" if cosine else ""
    m = lucid.VectorQuantize(K, D, kmeans_init=True, kmeans_iters=int(g["iters"]), use_cosine_sim=cosine).to(dev).eval()
    init = _t(g["init"], dev)
    m._codebook.sample_fn = lambda samples, num: samples[:, init[:num]]
    with torch.no_grad():
        _, _, (_, _, ind) = m(_t(g["x"], dev))
    assert float(m._codebook.initted) == 1.0
    assert np.array_equal(m._codebook.cluster_size[0].cpu().numpy(), g["bins" + sfx])
    ref = g["means" + sfx]
    assert np.abs(m._codebook.embed[0].cpu().numpy() - ref).max() <= 1e-5 * np.abs(ref).max()
    if not cosine:
        assert torch.equal(m._codebook.embed_avg, m._codebook.embed)
    assert np.array_equal(ind.cpu().numpy(), g["codes" + sfx])
    m._codebook.sample_fn = None                                   # initialised: the second forward samples nothing
    with torch.no_grad():
        m(_t(g["x"], dev))
