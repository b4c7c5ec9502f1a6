"""numpy restatement of residual quantization (include/dvq.h, "Residual quantization"), shared by tests/test_rq.py and
tests/test_rq_shapes.py.

`_restate` runs the reference's eval forward per depth with the oracle's assign; `chain`, `grad` and `embed` restate the header's
fp32 recipes of dvq_rq_step_f32 / dvq_rq_loss_f32, dvq_rq_backward_f32 and dvq_rq_embed_code_f32 for GIVEN codes, so a test of the
step kernels needs no search.  Every operation is one IEEE float32 operation of numpy, in the header's order.  A `geometry` is the
tuple (B, h, w, rH, rW, Dl): code grid h x w, latent [B, h rH, w rW, Dl], D = rH rW Dl channels per token, N = B h w tokens."""
import collections

import numpy as np
import torch

from dynamicvectorquantization_amd.rq import RQBottleneck

F32 = np.float32


def _to_code(x, rH, rW):
    B, H, W, Dl = x.shape
    return np.ascontiguousarray(x.reshape(B, H // rH, rH, W // rW, rW, Dl).transpose(0, 1, 3, 2, 4, 5)).reshape(B, H // rH, W // rW, -1)


def _to_latent(a, rH, rW, Dl):
    B, h, w, _ = a.shape
    return np.ascontiguousarray(a.reshape(B, h, w, rH, rW, Dl).transpose(0, 1, 3, 2, 4, 5)).reshape(B, h * rH, w * rW, Dl)


def _restate(oracle, x, books, rH, rW):
    """the reference's eval forward (quantize_rqvae.py:237-281) per depth: oracle assign on the residual, float32 updates.
    books = the K live rows of each depth's codebook -> (codes [B, h, w, d], out, agg_d (latent), loss)"""
    Dl = x.shape[-1]
    xc = _to_code(x, rH, rW)
    B, h, w, D = xc.shape
    xf = xc.reshape(-1, D)
    r = xf.copy()
    agg = np.zeros_like(xf)
    codes, means = [], []
    for E in books:
        c = oracle.vq_assign_nchw(r, E, want_zq=False)["codes"].reshape(-1)
        e = E[c]
        r = (r - e).astype(np.float32)
        agg = (agg + e).astype(np.float32)
        d = (xf - agg).astype(np.float32)
        means.append(np.float32(np.sum((d * d).astype(np.float64)) / d.size))
        codes.append(c)
    aggl = _to_latent(agg.reshape(B, h, w, D), rH, rW, Dl)
    out = (x + (aggl - x).astype(np.float32)).astype(np.float32)
    return np.stack(codes, -1).reshape(B, h, w, -1), out, aggl, float(np.mean(np.float64(means)))


def _books(rec, depth):
    if bool(rec["shared"]):
        return [rec["weight.0"][:-1]] * depth
    return [rec["weight.%d" % i][:-1] for i in range(depth)]


def _module(rec, dev=None):
    n_embed, decay = [int(k) for k in rec["n_embed"]], [float(v) for v in rec["decay"]]
    shared = bool(rec["shared"])
    rq = RQBottleneck(tuple(int(v) for v in rec["latent_shape"]), tuple(int(v) for v in rec["code_shape"]),
                      n_embed[0] if shared else n_embed, decay=decay[0] if shared else decay, shared_codebook=shared,
                      restart_unused_codes=bool(rec["restart"]))
    with torch.no_grad():
        for i, cb in enumerate(rq.codebooks[:1] if shared else rq.codebooks):
            cb.weight.copy_(torch.from_numpy(rec["weight.%d" % i]))
            cb.embed_ema.copy_(cb.weight[:-1])
            cb.cluster_size_ema.zero_()
    return rq if dev is None else rq.to(dev)


def same_bits(a, b):
    """equality of the uint32 views of two float32 arrays: -0 != +0, NaN payloads compare"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == np.float32 and b.dtype == np.float32, (a.dtype, b.dtype)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint32), b.view(np.uint32)))


def _rows(E, c):
    """E[c] with a NaN row where c is outside [0, len(E))"""
    ok = (c >= 0) & (c < E.shape[0])
    e = E[np.where(ok, c, 0)].astype(F32)
    e[~ok] = np.nan
    return e


Chain = collections.namedtuple("Chain", "residuals agg out s loss means")


def chain(x, books, codes, rH, rW, want_residuals=True):
    """dvq_rq_step_f32 for i = 0 .. depth-1 and dvq_rq_loss_f32 with GIVEN codes [N, depth] (books[i] = the K_i rows step i may
    gather) -> residuals [r_1 .. r_{depth-1}] ([N, D], code layout; empty without want_residuals), agg_d and out (latent layout),
    s ([N, D], code layout), the loss and its per-depth means (float32)"""
    assert x.dtype == np.float32
    Dl = x.shape[-1]
    xc = _to_code(x, rH, rW)
    B, h, w, D = xc.shape
    N, depth = B * h * w, len(books)
    codes = np.asarray(codes).reshape(N, depth)
    xf = xc.reshape(N, D)
    r = xf
    agg = np.zeros((N, D), F32)                                  # agg_0 = +0
    s = None
    residuals, means = [], []
    for i, E in enumerate(books):
        e = _rows(np.asarray(E, F32), codes[:, i])
        agg = agg + e
        if want_residuals and i + 1 < depth:
            r = r - e
            residuals.append(r)
        d = xf - agg
        sq = d * d
        assert agg.dtype == d.dtype == sq.dtype == np.float32
        means.append(F32(np.sum(sq.astype(np.float64)) / (float(N) * D)))
        s = d if i == 0 else s + d
    acc = F32(0.0)
    for m in means:
        acc = F32(acc + m)
    loss = F32(acc / F32(depth))
    aggl = _to_latent(agg.reshape(B, h, w, D), rH, rW, Dl)
    out = x + (aggl - x)
    assert out.dtype == np.float32 and s.dtype == np.float32
    return Chain(residuals, aggl, out, s, loss, means)


def grad(g_out, g_loss, s, N, D, depth, geometry):
    """dvq_rq_backward_f32: fl(g_out + fl(fl(g_loss fl32(2 / (N D depth))) s)) in latent layout; g_out [B, H, W, Dl] or None,
    g_loss a number or None (None = zero); s [N, D] from `chain`"""
    B, h, w, rH, rW, Dl = geometry
    assert N == B * h * w and D == rH * rW * Dl and s.shape == (N, D) and s.dtype == np.float32
    coef = F32(2.0 / (float(N) * D * depth))
    c0 = F32(0.0) if g_loss is None else F32(F32(g_loss) * coef)
    sl = _to_latent(s.reshape(B, h, w, D), rH, rW, Dl)
    go = np.zeros_like(sl) if g_out is None else np.asarray(g_out, F32).reshape(sl.shape)
    g = go + c0 * sl
    assert g.dtype == np.float32
    return g


def embed(books_with_padding, codes, mode, j, geometry):
    """dvq_rq_embed_code_f32 (books_with_padding[t] = the K_t rows a code of depth t may address), in latent layout:
    'sum' fl(...fl(+0 + e_0)... + e_j) [B, H, W, Dl]; 'select' e_j [B, H, W, Dl]; 'each' e_t, t <= j [B, H, W, j + 1, Dl];
    a code outside [0, K_t) gives a NaN row"""
    B, h, w, rH, rW, Dl = geometry
    N, D = B * h * w, rH * rW * Dl
    codes = np.asarray(codes).reshape(N, -1)
    lat = lambda a: _to_latent(a.reshape(B, h, w, D), rH, rW, Dl)
    rows = lambda t: _rows(np.asarray(books_with_padding[t], F32), codes[:, t])
    if mode == "select":
        return lat(rows(j))
    if mode == "each":
        return np.ascontiguousarray(np.stack([lat(rows(t)) for t in range(j + 1)], axis=-2))
    assert mode == "sum"
    acc = np.zeros((N, D), F32)
    for t in range(j + 1):
        acc = acc + rows(t)
    assert acc.dtype == np.float32
    return lat(acc)
