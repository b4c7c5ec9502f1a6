"""Float64 restatement of GumbelQuantize's backward in its hard form (csrc/vq_gumbel_backward.hip, quantize.gumbel_quantize), the
seeded gradients of the test cases and the rules of comparison.  numpy and torch on the CPU only.

Per token n, from the logits l [N, K] (the kernel's fp32 bits, or float64 logits), the variates q, u_k = embed_k . G_n, the scalar
g_kl = dL/dkl, tau and kl_K:

    s    = (l - log q) / tau                  (q None: l / tau)
    y    = softmax(s),  p = softmax(l),  delta = sum_k y_k u_k,  KL_n = sum_k p_k log(p_k kl_K)
    dl_k = y_k (u_k - delta) / tau + (g_kl / N) p_k (log p_k + log kl_K - KL_n)       (a term with p_k == 0 is 0)

A token whose logits are all -inf, or hold a NaN, has NaN in every dl_k (numpy's own arithmetic gives that: l - max l is NaN).
`torch_chain` is the reference's op sequence under torch autograd -- F.gumbel_softmax(hard=True)'s arithmetic, the one-hot einsum, the
KL term with its 1e-10 -- with the logits as the leaf: in float64 it checks the restatement, in float32 it is the baseline of the
tolerance (tests/test_gumbel_train_cases.py).

Rules.  A case's error is max |dl - dl64| / max |dl64| over its finite entries; where dl64 is identically zero (K = 1; all codes but
one at -inf) the denominator is max |u| / tau, and without u the kernel's zeros are exact.  Bound: BOUND = 8 ERR_REF, ERR_REF = 2.4e-6 the
largest error of the float32 torch chain on the CPU over the table and the two mixes below (the project's 8x rule).
Every token is compared: the codes are an input here (the forward's), so no near tie can move a gradient.
"""
import collections

import numpy as np
import torch

from tests import _score_cases as C

ERR_REF = 2.4e-6
BOUND = 1.9e-5                                      # 8 ERR_REF
# (name, with u, g_kl)
MIXES = (("zq+kl", True, 0.35), ("kl", False, 1.0), ("zq", True, None))
BASELINE_MIXES = MIXES[:2]                          # what ERR_REF was measured over


def dl64(l, q, u, g_kl, tau, kl_K):
    """[N, K] float64.  l [N, K] (fp32 bits or float64), q [N, K] or None, u [N, K] or None, g_kl a float or None"""
    l = np.asarray(l, np.float64)
    N = l.shape[0]
    out = np.zeros_like(l)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        if u is not None:
            s = (l if q is None else l - np.log(np.asarray(q, np.float64))) / float(tau)
            e = np.exp(s - s.max(axis=1, keepdims=True))
            y = e / e.sum(axis=1, keepdims=True)
            u = np.asarray(u, np.float64)
            delta = np.where(y != 0.0, y * u, 0.0).sum(axis=1, keepdims=True)
            delta = np.where(np.isnan(y).any(axis=1, keepdims=True), np.nan, delta)
            out = out + y * (u - delta) / float(tau)
        if g_kl is not None:
            x = l - l.max(axis=1, keepdims=True)
            e = np.exp(x)
            S = e.sum(axis=1, keepdims=True)
            p = e / S
            logp = x - np.log(S)
            kl_n = np.where(p != 0.0, p * (logp + np.log(float(kl_K))), 0.0).sum(axis=1, keepdims=True)
            t = np.where(p != 0.0, p * (logp + np.log(float(kl_K)) - kl_n), 0.0)
            t = np.where(np.isnan(p).any(axis=1, keepdims=True), np.nan, t)
            out = out + (float(g_kl) / N) * t
    return out


def torch_chain(l, q, E, G, g_kl, tau, kl_K, dtype):
    """d loss / d l [N, K] by torch autograd of the reference's ops, loss = sum(z_q G) + g_kl kl, everything in `dtype`:
    l [N, K] the leaf, q [N, K] or None, E [K, d], G [N, d] or None (no z_q term), g_kl a float or None"""
    lt = torch.tensor(np.asarray(l), dtype=dtype, requires_grad=True)
    loss = 0.0
    if G is not None:
        gum = 0.0 if q is None else -torch.tensor(np.asarray(q), dtype=dtype).log()
        y_soft = ((lt + gum) / tau).softmax(1)
        index = y_soft.max(1, keepdim=True)[1]
        y_hard = torch.zeros_like(lt).scatter_(1, index, 1.0)
        soft_one_hot = y_hard - y_soft.detach() + y_soft
        z_q = torch.einsum("nk,kd->nd", soft_one_hot, torch.tensor(np.asarray(E), dtype=dtype))
        loss = loss + (z_q * torch.tensor(np.asarray(G), dtype=dtype)).sum()
    if g_kl is not None:
        qy = lt.softmax(1)
        loss = loss + float(g_kl) * torch.sum(qy * torch.log(qy * float(kl_K) + 1e-10), dim=1).mean()
    loss.backward()
    return lt.grad.numpy().astype(np.float64)


def error(got, want, u, tau):
    """(normalised maximum error over the finite entries of `want`, the NaN patterns agree): the rule of the docstring"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    same_nan = bool(np.array_equal(np.isnan(got), nan))
    if nan.all():
        return 0.0, same_nan
    scale = float(np.abs(want[~nan]).max())
    if scale == 0.0:
        scale = 0.0 if u is None else float(np.abs(np.asarray(u, np.float64)).max()) / float(tau)
    err = float(np.abs(got[~nan] - want[~nan]).max()) if same_nan else float("inf")
    if scale == 0.0:
        return (0.0 if err == 0.0 else float("inf")), same_nan
    return err / scale, same_nan


def train_inputs(case, oracle):
    """gumbel_inputs(case) and, cached with it: qrows [N, K] or None, G [N, d] ~ N(0, 1) (seeded by the case), u32 [N, K] = fl32(G E^T
    formed in float64) -- the kernel's input -- and per mix name the float64 dl [N, K] from (l32, q, u32)"""
    def make():
        inp = C.gumbel_inputs(case, oracle)
        N = C.ntokens(case.shape)
        rng = np.random.default_rng(case.seed + 70000)
        G = rng.standard_normal((N, case.d)).astype(np.float32)
        u32 = (G.astype(np.float64) @ inp["E"].astype(np.float64).T).astype(np.float32)
        qrows = None if inp["q"] is None else C.to_rows(inp["q"])
        out = {"G": G, "u32": u32, "qrows": qrows}
        for name, with_u, g_kl in MIXES:
            out[name] = dl64(inp["l32"], qrows, u32 if with_u else None, g_kl, case.tau, inp["kl_K"])
        return out
    return C.cached(("gumbel_train", case.name), make)


# ---- the backward's code loop over several chunks ------------------------------------------------------------------------------
# The kernel's lane takes its codes in chunks of 8, one code per lane half and wave apart: a chunk spans 256 codes in the 16-wave form
# (below 1024 workgroups of 32 tokens) and 64 in the 4-wave form.  The table above stays within one chunk (K <= 160; K = 8 in the
# 4-wave form), so these cases feed logits, q and u of several chunks straight to the kernel -- no projection, no oracle:
#   shape [B, K, HW]: 45 tokens x K = 600 (3 chunks, the last partial) and 1100 (5 chunks): the 16-wave form;
#                     1025 x 33 = 33 825 tokens (1058 workgroups, the last partial) x K = 264 (5 chunks, the last partial): the 4-wave form
#   kind   "normal": logits of standard deviation 3;  "ramp_up": + 120 k / K (the span of the table's ramp, 0.75 x 160), the maximum rises in every chunk and the
#          early terms underflow;  "inf_lead": -inf on the codes of every lane's whole first chunk and a few beyond (a later chunk brings the
#          first finite value), and rows 3 and 7 -inf everywhere (NaN rows)
ChunkCase = collections.namedtuple("ChunkCase", "name B K HW noise tau kind lead seed")
CHUNK_CASES = tuple(
    ChunkCase("chunks-%dx%dx%d-%s-%s" % (B, K, HW, kind, "q" if noise else "noq"), B, K, HW, noise, tau, kind, lead, 9700 + i)
    for i, (B, K, HW, lead, kind, noise, tau) in enumerate(
        (B, K, HW, lead, kind, noise, tau)
        for B, K, HW, lead in ((3, 600, 15, 300), (3, 1100, 15, 300), (1025, 264, 33, 80))
        for kind, noise, tau in (("normal", False, 0.5), ("ramp_up", True, 1.0), ("inf_lead", True, 0.5))))
CHUNK_BY_NAME = {c.name: c for c in CHUNK_CASES}
# the float32 torch chain's own error over THESE cases and the three mixes (`torch_chain_u` on the CPU; 3.62e-6 at
# chunks-1025x264x33-ramp_up-q, kl: more terms per sum than the table has).  The kernel is held to BOUND here too, which is below 8 x this.
CHUNK_ERR_REF = 3.7e-6
CHUNK_NAN_ROWS = (3, 7)


def chunk_inputs(case):
    """dict: l32, qrows (or None), u32 [N, K] float32 token rows, kl_K, dead (bool [K]: codes at -inf) and per mix the float64 dl"""
    def make():
        rng = np.random.default_rng(case.seed)
        N, K = case.B * case.HW, case.K
        l = (3.0 * rng.standard_normal((N, K))).astype(np.float32)
        dead = np.zeros(K, bool)
        if case.kind == "ramp_up":
            l = l + np.float32(120.0 / K) * np.arange(K, dtype=np.float32)[None, :]
        elif case.kind == "inf_lead":
            dead[:case.lead] = True
            l[:, dead] = -np.inf
            l[list(CHUNK_NAN_ROWS)] = -np.inf
        qrows = np.maximum(rng.standard_exponential((N, K)).astype(np.float32), np.float32(1e-30)) if case.noise else None
        u32 = (4.0 * rng.standard_normal((N, K))).astype(np.float32)
        out = {"l32": l, "qrows": qrows, "u32": u32, "kl_K": float(K), "dead": dead}
        for name, with_u, g_kl in MIXES:
            out[name] = dl64(l, qrows, u32 if with_u else None, g_kl, case.tau, float(K))
        return out
    return C.cached(("gumbel_chunks", case.name), make)


def torch_chain_u(l, q, u, g_kl, tau, kl_K, dtype):
    """torch_chain with u given instead of (E, G): the z_q term's loss is sum(soft_one_hot u), whose gradient is the einsum's"""
    lt = torch.tensor(np.asarray(l), dtype=dtype, requires_grad=True)
    loss = 0.0
    if u is not None:
        gum = 0.0 if q is None else -torch.tensor(np.asarray(q), dtype=dtype).log()
        y_soft = ((lt + gum) / tau).softmax(1)
        index = y_soft.max(1, keepdim=True)[1]
        y_hard = torch.zeros_like(lt).scatter_(1, index, 1.0)
        loss = loss + ((y_hard - y_soft.detach() + y_soft) * torch.tensor(np.asarray(u), dtype=dtype)).sum()
    if g_kl is not None:
        qy = lt.softmax(1)
        loss = loss + float(g_kl) * torch.sum(qy * torch.log(qy * float(kl_K) + 1e-10), dim=1).mean()
    loss.backward()
    return lt.grad.numpy().astype(np.float64)


def logits_shape(case):
    return (case.shape[0], case.K) + tuple(case.shape[2:])


def grads64(z, W, b, E, q, tau, kl_K, codes, G, g_kl):
    """End to end in float64, the forward's codes AS GIVEN: z [B, C, H, W], W [K, C], b [K], E [K, d], q [B, K, H, W] or None,
    codes [B, H, W], G = dL/dz_q [B, d, H, W], g_kl = dL/dkl -> (dz [B, C, H, W], dW [K, C], db [K], dE [K, d])"""
    z64, W64, G64 = z.astype(np.float64), W.astype(np.float64), G.astype(np.float64)
    B, Cc, H, Wd = z.shape
    K = W.shape[0]
    l = np.einsum("bchw,kc->bkhw", z64, W64) + b.astype(np.float64)[None, :, None, None]
    rows = lambda t: np.ascontiguousarray(t.reshape(B, t.shape[1], -1).transpose(0, 2, 1)).reshape(B * H * Wd, t.shape[1])
    u = rows(G64) @ E.astype(np.float64).T
    dl = dl64(rows(l), None if q is None else rows(q), u, g_kl, tau, kl_K)
    dz = (dl @ W64).reshape(B, H * Wd, Cc).transpose(0, 2, 1).reshape(z.shape)
    dW = dl.T @ rows(z64)
    db = dl.sum(axis=0)
    dE = np.zeros(E.shape, np.float64)
    np.add.at(dE, np.asarray(codes).reshape(-1), rows(G64))
    return dz, dW, db, dE
