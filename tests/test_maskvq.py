"""MaskVectorQuantize / VectorQuantize (quantize.py), the scored / sampled assign (dvq_vq_score_assign_f32) and quantisation from
given codes (dvq_vq_apply_codes_*_f32) against the reference's own modules on the CPU (tests/golden/maskvq_*.npz, written by
tools/gen_golden_maskvq.py) and the numpy restatement tests/_maskvq_ref.py, whose docstring derives the skip rule: at temp = 0
every code must match; at temp > 0 a code may differ only where the float64 top-2 gap of the perturbed scores is below
4 G_ERR + ulp32(best), for at most 0.1 % of a fixture's tokens."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _maskvq_ref as R
from dynamicvectorquantization_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_FIX = {}
NEW = ("dvq_vq_score_assign_f32", "dvq_vq_apply_codes_nchw_f32", "dvq_vq_apply_codes_flat_f32")


def _fixture(tag):
    """loaded once and shared read-only"""
    if tag not in _FIX:
        g = R.load(tag)
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _FIX[tag] = g
    return _FIX[tag]


def _rows(g):
    """the reference's `flatten` [N, D] of the fixture's module input"""
    x, layout = g["x"], str(g["layout"])
    if layout == "nchw":
        return np.ascontiguousarray(x.reshape(x.shape[0], x.shape[1], -1).transpose(0, 2, 1)).reshape(-1, x.shape[1])
    if layout == "bdn":
        return np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(-1, x.shape[1])
    return x.reshape(-1, x.shape[-1])


def _temps(g):
    """[(suffix, temp, u or None)]"""
    out = [("0", 0.0, None)]
    if "temp1" in g:
        out.append(("1", float(g["temp1"]), g["u1"]))
    return out


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_declared_and_exported():
    from dynamicvectorquantization_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvq.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.EXPORTS
    assert _lib.lib.dvq_version() >= 1200


def test_abi_validation_without_gpu():
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    a = 256                                                        # a "pointer" that passes the alignment checks

    def score(x=a, prep=a, B=2, D=256, HW=64, K=96, metric=0, temp=1.0, u=0, un=0, codes=a):
        return L.dvq_vq_score_assign_f32(x, prep, B, D, HW, K, metric, temp, u, un, codes, 0)

    for null in ("x", "prep", "codes"):
        assert score(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert score(u=a, un=128 * 96 - 1) == EINVAL and b"u has" in L.dvq_last_error_string()     # a u of the wrong size
    assert score(u=a, un=128 * 96 + 96) == EINVAL
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert score(u=a, un=128 * 96, temp=bad) == EINVAL and b"temp" in L.dvq_last_error_string()
    assert score(metric=2) == EINVAL
    assert score(B=0) == EINVAL
    assert score(D=100) == EUNSUPPORTED and b"zero channels" in L.dvq_last_error_string()

    def apply(z=a, codes=a, cb=a, mask=0, B=2, D=256, HW=64, K=96, zq=a, loss=0, ws=0, wsb=0):
        return L.dvq_vq_apply_codes_nchw_f32(z, codes, cb, mask, B, D, HW, K, 0.25, zq, loss, ws, wsb, 0)

    for null in ("z", "codes", "cb"):
        assert apply(**{null: 0}) == EINVAL
    assert apply(zq=0) == EINVAL
    assert apply(D=100) == EUNSUPPORTED
    need = L.dvq_vq_assign_workspace_bytes(2, 256, 64, 96, 0)
    assert apply(loss=a, ws=a, wsb=need - 1) == EWORKSPACE and apply(loss=a, ws=0, wsb=need) == EWORKSPACE
    assert L.dvq_vq_apply_codes_flat_f32(a, a, a, 0, 0, 256, 96, 0.25, a, 0, 0, 0, 0) == EINVAL


@pytest.mark.parametrize("tag", R.FIXTURES)
def test_restatement_reproduces_the_reference(tag):
    """tests/_maskvq_ref.py from the reference's own fp32 scores and the replayed u gives the reference's codes, skip rules
    applied, and its loss from the gathered rows; the skip sets stay under the cap"""
    g = _fixture(tag)
    dist = g["dist"]
    assert np.array_equal(R.argmax_torch(dist), g["codes0"].reshape(-1))
    for sfx, temp, u in _temps(g)[1:]:
        skip = R.skip_sampled(dist, temp, u)
        assert np.array_equal(skip, g["skip" + sfx]) and skip.mean() <= R.SKIP_CAP
        mine = R.argmax_torch(R.perturbed(dist, temp, u))
        assert np.array_equal(mine[~skip], g["codes" + sfx].reshape(-1)[~skip])
    rows = _rows(g)
    for sfx, _, _ in _temps(g):
        codes = g["codes" + sfx].reshape(-1)
        want = float(g["loss" + sfx])
        mask = g["mask"].reshape(-1) if "mask" in g else None
        got = R.loss_ref(rows, g["E"][codes], float(g["beta"]), mask)
        assert (np.isnan(want) and np.isnan(got)) or abs(got - want) <= 1e-5 * abs(want)


def test_new_classes_take_the_generic_encode_path():
    """no routed / conv-routed / folded form for these classes: _can_route & co answer False rather than raise"""
    from dynamicvectorquantization_amd import encode
    from dynamicvectorquantization_amd.quantize import MaskVectorQuantize, VectorQuantize
    h = torch.zeros(1, 256, 4, 4)
    conv = torch.nn.Conv2d(256, 256, 1)
    for m in (MaskVectorQuantize(96, 256).eval(), VectorQuantize(96, 256).eval()):
        assert encode._can_route(m, None, h, h) is False
        assert encode._can_route_conv(m, conv, h, h) is False
        assert encode._can_fold(m, conv, h, h) is False
        assert encode._can_fuse_vqgan(m, conv, h) is False


def test_state_dict_and_cpu_tensors_raise():
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import MaskVectorQuantize, VectorQuantize
    g = _fixture("a_l2_masked")
    for m in (MaskVectorQuantize(96, 256), VectorQuantize(96, 256, use_cosine_distance=True)):
        assert sorted(m.state_dict().keys()) == list(g["state_keys"]) == ["cluster_size", "embedding.weight", "initted"]
        assert float(m.initted) == 1.0 and tuple(m.cluster_size.shape) == (1, 96)
        with pytest.raises(_lib.DvqError):
            m(torch.zeros(1, 256, 2, 2))
    m = MaskVectorQuantize(8, 64, kmeans_init=True)
    assert float(m.initted) == 0.0 and float(m.embedding.weight.detach().abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- GPU

def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _operands(g):
    """(token rows [N, D], codebook rows, metric) the kernel scores for this fixture: the reference's own operands"""
    from dynamicvectorquantization_amd import _lib
    metric = str(g["metric"])
    if metric == "l2":
        return _rows(g), g["E"], _lib.METRIC_L2
    return g["xn"], g["wn"], (_lib.METRIC_DOT if metric == "cos" else _lib.METRIC_L2)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", R.FIXTURES)
def test_score_assign_codes(tag, dev):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, score_assign
    g = _fixture(tag)
    rows, book, metric = _operands(g)
    prep = _CodebookPrep()
    for sfx, temp, u in _temps(g):
        got = score_assign(_t(rows, dev), _t(book, dev), prep, metric, temp, _t(u, dev))
        assert got.dtype == torch.int64 and tuple(got.shape) == (rows.shape[0],)
        got, want = got.cpu().numpy(), g["codes" + sfx].reshape(-1)
        if u is None:
            assert np.array_equal(got, want)                     # exact for every token, ties and NaN included
        else:
            skip = R.skip_sampled(g["dist"], temp, u)
            print("%s temp %g: %d of %d tokens in the skip set, %d differ" % (tag, temp, skip.sum(), skip.size, (got != want).sum()))
            assert skip.mean() <= R.SKIP_CAP
            assert np.array_equal(got[~skip], want[~skip])
            # an unaligned u (K % 4 == 0 but the rows start 4 bytes off): the scalar reads, the same codes
            buf = torch.empty(u.size + 1, device=dev)
            buf[1:].copy_(_t(u, dev).reshape(-1))
            again = score_assign(_t(rows, dev), _t(book, dev), prep, metric, temp, buf[1:].view(u.shape))
            assert np.array_equal(again.cpu().numpy(), got)


@pytest.mark.gpu
def test_nchw_equals_row_major(dev):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, score_assign
    g = _fixture("a_l2_masked")
    prep, E = _CodebookPrep(), _t(g["E"], dev)
    x, rows, u = _t(g["x"], dev), _t(_rows(g), dev), _t(g["u1"], dev)
    for metric in (0, 1):
        for temp, uu in ((0.0, None), (float(g["temp1"]), u)):
            a = score_assign(x, E, prep, metric, temp, uu)
            b = score_assign(rows, E, prep, metric, temp, uu)
            assert tuple(a.shape) == (2, 8, 8) and torch.equal(a.reshape(-1), b)
    # K not a multiple of 4: scalar reads of u, a ragged last tile
    K = 94
    u94 = torch.zeros(128, K, device=dev).uniform_(0, 1)
    a = score_assign(x, E[:K].contiguous(), _CodebookPrep(), 0, 1.0, u94)
    want = R.argmax_torch(R.perturbed(g["dist"][:, :K], 1.0, u94.cpu().numpy()))
    skip = R.skip_sampled(g["dist"][:, :K], 1.0, u94.cpu().numpy())
    assert skip.mean() <= 0.01 and np.array_equal(a.reshape(-1).cpu().numpy()[~skip], want[~skip])


@pytest.mark.gpu
@pytest.mark.parametrize("tag", ("a_l2_masked", "b_l2_flat"))
def test_apply_codes(tag, dev):
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, apply_codes, score_assign, vq_assign
    g = _fixture(tag)
    nchw = str(g["layout"]) == "nchw"
    z = _t(g["x"] if nchw else _rows(g), dev)
    E, mask, beta = _t(g["E"], dev), _t(g.get("mask"), dev), float(g["beta"])
    prep = _CodebookPrep()
    zq_a, codes_a, loss_a = vq_assign(z, E, prep, mask, beta)
    zq, loss = apply_codes(z, codes_a, E, _CodebookPrep(), mask, beta)
    assert torch.equal(zq, zq_a)                                  # bit-identical
    assert torch.allclose(loss, loss_a, rtol=1e-5, atol=0.0), (loss, loss_a)
    assert apply_codes(z, codes_a, E, prep, mask, beta, want_zq=False)[0] is None
    assert apply_codes(z, codes_a, E, prep, mask, beta, want_loss=False)[1] is None
    # temp > 0: the kernel's sampled codes, then x_q / loss against the reference's
    temp, u = float(g["temp1"]), g["u1"]
    codes = score_assign(z, E, prep, 0, temp, _t(u, dev))
    zq, loss = apply_codes(z, codes, E, prep, mask, beta)
    skip = R.skip_sampled(g["dist"], temp, u)
    keep = ~skip
    got = zq.cpu().numpy()
    rows = lambda a: np.ascontiguousarray(a.reshape(a.shape[0], a.shape[1], -1).transpose(0, 2, 1)).reshape(-1, a.shape[1]) if nchw else a.reshape(-1, a.shape[-1])
    assert np.array_equal(rows(got)[keep].view(np.uint32), rows(g["xq1"])[keep].view(np.uint32))
    want = float(g["loss1"])
    ratio = 1.0 if mask is None else 1.0 / float(g["mask"].mean())
    assert abs(float(loss[1]) * ratio - want) <= 1e-5 * abs(want), (float(loss[1]) * ratio, want)


def _module(g, dev, **extra):
    from dynamicvectorquantization_amd import quantize as Q
    cls = Q.MaskVectorQuantize if str(g["cls"]) == "mask" else Q.VectorQuantize
    layout, metric = str(g["layout"]), str(g["metric"])
    kw = {}
    if layout != "nchw":
        kw.update(accept_image_fmap=False, channel_last=(layout == "flat"))
    if metric == "cos":
        kw["use_cosine_sim"] = True
    if metric == "cosdist":
        kw["use_cosine_distance"] = True
    kw.update(extra)
    m = cls(int(g["K"]), int(g["D"]), **kw).to(dev).eval()
    m.embedding.weight.data.copy_(_t(g["E"], dev))
    m.invalidate_codebook_cache()
    return m


def _forward(m, g, dev, temp, u, x=None):
    """the module's forward with the fixture's uniforms in place of its own draw"""
    if u is not None:
        ut = _t(u, dev)
        m._draw_uniform = lambda N, K, device: ut.reshape(N, K)
    x = _t(g["x"], dev) if x is None else x
    if "mask" in g:
        return m(x, temp=temp, codebook_mask=_t(g["mask"], dev))
    return m(x, temp=temp)


@pytest.mark.gpu
@pytest.mark.parametrize("tag", R.FIXTURES)
def test_module_matches_the_reference(tag, dev):
    g = _fixture(tag)
    m = _module(g, dev)
    assert sorted(m.state_dict().keys()) == list(g["state_keys"])
    cosine = str(g["metric"]) != "l2"
    for sfx, temp, u in _temps(g):
        with torch.no_grad():
            xq, loss, (a, b, ind) = _forward(m, g, dev, temp, u)
        assert a is None and b is None and ind.dtype == torch.int64
        want = g["codes" + sfx]
        assert tuple(ind.shape) == want.shape and tuple(xq.shape) == g["xq" + sfx].shape
        got = ind.cpu().numpy().reshape(-1)
        N = got.size
        if tag.startswith("d_") or not (cosine or u is not None):
            skip = np.zeros(N, bool)                              # every token, ties and NaN included
        elif u is None:
            skip = R.skip_cosine_hard(g["dist"])
        else:
            skip = R.skip_sampled(g["dist"], temp, u, cosine_end_to_end=cosine)
        assert skip.mean() <= R.SKIP_CAP
        keep = ~skip
        assert np.array_equal(got[keep], want.reshape(-1)[keep])
        layout = str(g["layout"])
        tok = lambda t: (np.moveaxis(t.reshape(t.shape[0], t.shape[1], -1), 1, 2).reshape(N, -1) if layout != "flat" else t.reshape(N, -1))
        gx, wx = tok(xq.cpu().numpy()), tok(g["xq" + sfx])
        assert np.array_equal(gx[keep].view(np.uint32), wx[keep].view(np.uint32))
        wl, gl = float(g["loss" + sfx]), float(loss)
        print("%s temp %g: loss %.9g, reference %.9g" % (tag, temp, gl, wl))
        assert (np.isnan(wl) and np.isnan(gl)) or abs(gl - wl) <= 1e-5 * abs(wl)


@pytest.mark.gpu
@pytest.mark.parametrize("temp", (0.0, 1.0))
def test_gradients(temp, dev):
    """d loss / d x and d loss / d embedding.weight against the torch-op restatement of the reference graph on the GPU with the
    kernel's codes forced; the straight-through d x_q / d x is the identity"""
    g = _fixture("a_l2_masked")
    m = _module(g, dev).train()
    beta = float(g["beta"])
    x = _t(g["x"], dev).requires_grad_(True)
    mask = _t(g["mask"], dev)
    G = _t(synth.normal(8190, g["x"].shape), dev)
    xq, loss, (_, _, ind) = _forward(m, g, dev, temp, g["u1"] if temp > 0 else None, x=x)
    gx_l, gw_l = torch.autograd.grad(loss, (x, m.embedding.weight), retain_graph=True)
    gx_q, = torch.autograd.grad((xq * G).sum(), x, retain_graph=True)
    assert torch.equal(gx_q, G)                                   # identity
    gx_both, gw_both = torch.autograd.grad(loss * 3.0 + (xq * G).sum(), (x, m.embedding.weight))
    # the reference graph (quantize_codebook_mask.py:80-135) in torch ops, codes forced
    x2 = _t(g["x"], dev).requires_grad_(True)
    w2 = m.embedding.weight.detach().clone().requires_grad_(True)
    xr = x2.permute(0, 2, 3, 1).reshape(2, 64, 256)
    mr = mask.permute(0, 2, 3, 1).reshape(2, 64, 1)
    e = torch.nn.functional.embedding(ind.reshape(2, 64), w2)
    ratio = 1 / torch.mean(mr)
    loss2 = ratio * beta * torch.mean((e.detach() - xr) ** 2 * mr) + ratio * torch.mean((e - xr.detach()) ** 2 * mr)
    xq2 = (xr + (e - xr).detach()).reshape(2, 8, 8, 256).permute(0, 3, 1, 2)
    rx_l, rw_l = torch.autograd.grad(loss2, (x2, w2), retain_graph=True)
    rx_both, rw_both = torch.autograd.grad(loss2 * 3.0 + (xq2 * G).sum(), (x2, w2))
    assert abs(float(loss.detach()) - float(loss2.detach())) <= 1e-5 * abs(float(loss2.detach()))
    for got, want in ((gx_l, rx_l), (gw_l, rw_l), (gx_both, rx_both), (gw_both, rw_both)):
        assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-6
    assert float(gw_l.abs().max()) > 0.0 and float(gx_l.abs().max()) > 0.0


@pytest.mark.gpu
def test_noise_comes_from_torchs_generator(dev):
    g = _fixture("a_l2_masked")
    m = _module(g, dev)
    x, mask = _t(g["x"], dev), _t(g["mask"], dev)
    N, K = 128, 96
    torch.manual_seed(4242)
    with torch.no_grad():
        _, _, (_, _, c1) = m(x, temp=1.0, codebook_mask=mask)
    after = torch.cuda.get_rng_state(dev)
    torch.manual_seed(4242)
    u = torch.zeros(N, K, device=dev).uniform_(0, 1)
    assert torch.equal(torch.cuda.get_rng_state(dev), after)      # exactly N * K uniforms were consumed
    torch.manual_seed(4242)
    with torch.no_grad():
        _, _, (_, _, c2) = m(x, temp=1.0, codebook_mask=mask)
        _, _, (_, _, c0) = m(x, temp=0.0, codebook_mask=mask)
    assert torch.equal(c1, c2)
    assert torch.equal(torch.cuda.get_rng_state(dev), after)      # temp == 0 draws nothing
    un = u.cpu().numpy()
    skip = R.skip_sampled(g["dist"], 1.0, un)
    want = R.argmax_torch(R.perturbed(g["dist"], 1.0, un))
    assert skip.mean() <= 0.01 and np.array_equal(c1.cpu().numpy().reshape(-1)[~skip], want[~skip])
    assert not torch.equal(c1, c0)


@pytest.mark.gpu
@pytest.mark.parametrize("K", (8, 12))
def test_kmeans_init(K, dev):
    """8 well-separated Gaussian clusters (centre distance >> spread), one sampled point per cluster; K = 12 adds four far-away
    sampled rows that attract nothing: empty clusters keep the sampled value"""
    from dynamicvectorquantization_amd.quantize import MaskVectorQuantize
    D, N = 64, 1024
    centres = synth.normal(8301, (8, D), 0.0, 4.0)
    labels = synth.randint(8302, (N,), 8)
    labels[:8] = np.arange(8)
    pts = (centres[labels] + synth.normal(8303, (N, D), 0.0, 0.05)).astype(np.float32)
    first = np.array([int(np.flatnonzero(labels == j)[0]) for j in range(8)])
    far = (1000.0 + synth.normal(8304, (4, D))).astype(np.float32)
    calls = []

    def sample_fn(samples, num):
        assert tuple(samples.shape) == (1, N, D) and num == K
        rows = samples[:, torch.as_tensor(first, device=samples.device)]
        if num > 8:
            rows = torch.cat([rows, torch.as_tensor(far, device=samples.device).unsqueeze(0)], dim=1)
        return rows

    m = MaskVectorQuantize(K, D, kmeans_init=True, kmeans_iters=3, accept_image_fmap=False, channel_last=True).to(dev).eval()
    m.sample_fn = sample_fn
    m.all_reduce_fn = lambda t: calls.append(tuple(t.shape))
    with torch.no_grad():
        xq, loss, (_, _, ind) = m(_t(pts.reshape(2, N // 2, D), dev), temp=0.)
    assert float(m.initted) == 1.0
    assert calls == [(1, K), (1, K, D)] * 3                        # bins and means, every iteration
    counts = np.bincount(labels, minlength=8)
    assert tuple(m.cluster_size.shape) == (1, K)
    assert np.array_equal(m.cluster_size.cpu().numpy()[0, :8], counts.astype(np.float32))
    assert np.all(m.cluster_size.cpu().numpy()[0, 8:] == 0)
    ref = np.stack([pts[labels == j].astype(np.float64).mean(axis=0) for j in range(8)])
    w = m.embedding.weight.detach().cpu().numpy()
    assert np.abs(w[:8] - ref).max() <= 1e-5 * np.abs(ref).max()
    assert np.array_equal(w[8:], far[:K - 8])                      # empty clusters keep the sampled rows
    assert np.array_equal(ind.cpu().numpy().reshape(-1), labels)
    with torch.no_grad():                                          # initialised: the second forward samples nothing
        m.sample_fn = None
        m(_t(pts.reshape(2, N // 2, D), dev), temp=0.)


@pytest.mark.gpu
def test_validation_and_padded_width(dev):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import MaskVectorQuantize, VectorQuantize, _CodebookPrep, score_assign
    g = _fixture("a_l2_masked")
    m = _module(g, dev)
    x = _t(g["x"], dev)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temp"):
            m(x, temp=bad)
    with pytest.raises(_lib.DvqError, match="rc=-1"):               # a u of the wrong size: the ABI's EINVAL
        score_assign(x, _t(g["E"], dev), _CodebookPrep(), 0, 1.0, torch.zeros(127, 96, device=dev))
    with pytest.raises(_lib.DvqError, match="codebook_dim 100"):
        MaskVectorQuantize(96, 100).to(dev)(torch.zeros(1, 100, 2, 2, device=dev))
    # D = 96 runs and equals the zero-padded D = 128 run bit for bit
    K, N = 96, 70
    E = synth.codebook_trained(K, 96, seed=8401)
    xr = np.ascontiguousarray(synth.z_tokens(E, 1, N, 1, 8402)[0, :, :, 0].T)
    Ep, xp = np.zeros((K, 128), np.float32), np.zeros((N, 128), np.float32)
    Ep[:, :96], xp[:, :96] = E, xr
    u = torch.zeros(N, K, device=dev).uniform_(0, 1)
    flat = dict(accept_image_fmap=False, channel_last=True)
    outs = []
    for Ei, xi in ((E, xr), (Ep, xp)):
        mm = MaskVectorQuantize(K, Ei.shape[1], **flat).to(dev).eval()
        mm.embedding.weight.data.copy_(_t(Ei, dev))
        mm._draw_uniform = lambda N_, K_, device: u
        with torch.no_grad():
            outs.append([mm(_t(xi.reshape(1, N, -1), dev), temp=t) for t in (0.0, 1.0)])
    for (xa, la, (_, _, ia)), (xb, lb, (_, _, ib)) in zip(*outs):
        assert torch.equal(ia, ib) and torch.equal(xa, xb[..., :96])
        assert bool((xb[..., 96:] == 0).all())
        assert abs(float(la) - float(lb) * 128.0 / 96.0) <= 1e-5 * abs(float(la))
    # the cosine metrics at a padded width: the kernel sees zero channels, the normalisation does not
    for cls, kw in ((MaskVectorQuantize, dict(use_cosine_sim=True)), (VectorQuantize, dict(use_cosine_distance=True))):
        mm = cls(K, 96, **flat, **kw).to(dev).eval()
        mm.embedding.weight.data.copy_(_t(E, dev))
        with torch.no_grad():
            xq, loss, (_, _, ind) = mm(_t(xr.reshape(1, N, 96), dev), temp=0.0)
        cos = torch.nn.functional.normalize(_t(xr, dev), dim=-1) @ torch.nn.functional.normalize(_t(E, dev), dim=-1).t()
        top = torch.gather(cos, 1, ind.reshape(N, 1)).reshape(N)
        assert float((cos.max(dim=1).values - top).max()) <= 1e-6 and torch.isfinite(loss)
