"""Residual quantization away from the reference's own geometry: code grids with h != w, divisors with rH != rW, Dl that is no
multiple of 4, zero-padded widths (D = 32, 96), depth 1, 2 and DVQ_RQ_MAX_DEPTH, more than 256 loss partials, the 2048-block cap,
the sign of zero, codes out of range, null gradients, a stale workspace and an empty batch.  tests/test_rq.py holds the reference's
geometries; the restatement of both files is tests/_rq_ref.py.

Goldens (tools/gen_golden_rq.py, the reference's own RQBottleneck; every third channel of every fifth codebook row and every
seventh element of x are -0.0 in the eval cases).  Generator seeds: 41 .. 46 in the order of the table, the first ones tried: the
oracle's codes equal the reference's at every token of every case.

  case  tag             latent / code          B   codebooks       h x w  rH x rW  Dl  D    N     depth  what it reaches
  G1    eval_r2x8_dl6   (6,40,6)/(3,5,3)       3   [40,72,100]     3x5    2x8      6   96   45    3      4-byte form by Dl % 4, padded width, N D % 1024 != 0
  G2    eval_r4x2_dl8   (20,6,8)/(5,3,2)       5   [50,64]         5x3    4x2      8   64   75    2      16-byte form at Dl = 8, one residual slot
  G3    eval_depth1     (3,7,32)/(3,7,1)       2   shared 33       3x7    1x1      32  32   42    1      depth 1, D = 32, h != w at divisor 1
  G4    eval_depth16    (4,6,16)/(2,3,16)      3   shared 48       2x3    2x2      16  64   18    16     DVQ_RQ_MAX_DEPTH
  G5    eval_r2x8_dl2   (2,16,2)/(1,2,2)       7   shared 20       1x2    2x8      2   32   14    2      Dl < 4, h = 1
  T1    train_r2x4      (6,20,8)/(3,5,3)       3   shared 40       3x5    2x4      8   64   45    3      training, shared codebook, non-square divisor
  S2    (no golden)     (20,6,8)/(5,3,2)       5   [64,64]         5x3    4x2      8   64   75    2      soft codes stack: codebooks of one size
  L1    (given codes)   (20,80,6)/(10,10,2)    32  [64,64]         10x10  2x8      6   96   3200  2      P = 300: a second, partial pass over the loss partials
  L2    (given codes)   (10,40,128)/(10,20,2)  48  [64,64]         10x20  1x2      128 256  9600  2      P capped at 2048: the grid-stride loops stride

`test_case_table_reaches_what_it_claims` checks the last column against the library and the launcher's source without a device.

The loss of a run is compared with `_rq_ref.chain` at (depth + 2) 2^-24 relative: the double sums differ from the exact ones by
about 2^-32, then one fp32 rounding per mean, at most depth - 1 in the non-negative fp32 sum of the means and one in the division.
Every comparison called bit-exact is `same_bits` (uint32 views).

What the cases see.  In `rq_latent_row`, exchanging a and c or h and w literally indexes out of bounds wherever rH != rW or h != w,
so the exchanges were tried in their in-bounds forms on a scratch build: the cell index read as c rH + a fails G1, G2, G4, G5, T1,
L1 and the out-of-range test (it is the identity at rH = 1, so L2 passes); the token index read as ww h + hh fails G1, G2, G4, T1,
L1 and L2 (the identity at h = 1, so G5 passes).  G3 has divisor 1 x 1, where the function returns early."""
import collections
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib, synth
from dynamicvectorquantization_amd.rq import RQBottleneck
from tests import _rq_ref as R
from tests._rq_ref import _books, _restate, _to_code, _to_latent, same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
U = 2.0 ** -24

Case = collections.namedtuple("Case", "tag latent code B n_embed shared claims")
CASES = {
    "G1": Case("eval_r2x8_dl6", (6, 40, 6), (3, 5, 3), 3, [40, 72, 100], False, {"vw1", "ragged"}),
    "G2": Case("eval_r4x2_dl8", (20, 6, 8), (5, 3, 2), 5, [50, 64], False, {"vw4", "depth2"}),
    "G3": Case("eval_depth1", (3, 7, 32), (3, 7, 1), 2, [33], True, {"vw4", "depth1"}),
    "G4": Case("eval_depth16", (4, 6, 16), (2, 3, 16), 3, [48] * 16, True, {"vw4", "depth16"}),
    "G5": Case("eval_r2x8_dl2", (2, 16, 2), (1, 2, 2), 7, [20] * 2, True, {"vw1", "depth2"}),
    "T1": Case("train_r2x4", (6, 20, 8), (3, 5, 3), 3, [40] * 3, True, {"vw4"}),
    "S2": Case(None, (20, 6, 8), (5, 3, 2), 5, [64, 64], False, {"vw4", "depth2"}),
    "L1": Case(None, (20, 80, 6), (10, 10, 2), 32, [64, 64], False, {"vw1", "partials>256", "depth2"}),
    "L2": Case(None, (10, 40, 128), (10, 20, 2), 48, [64, 64], False, {"vw4", "capped", "depth2"}),
}
EVAL = ("G1", "G2", "G3", "G4", "G5")
GIVEN = EVAL + ("L1", "L2")

Geom = collections.namedtuple("Geom", "B h w rH rW Dl D N depth")


def _geom(case, B=None):
    (H, W, Dl), (h, w, depth) = case.latent, case.code
    B = case.B if B is None else B
    rH, rW = H // h, W // w
    return Geom(B, h, w, rH, rW, Dl, rH * rW * Dl, B * h * w, depth)


def _geometry(g):
    return (g.B, g.h, g.w, g.rH, g.rW, g.Dl)


_CACHE = {}


def _cached(key, make):
    """computed once, shared by the tests that need it and never written to afterwards"""
    if key not in _CACHE:
        val = make()
        for a in (val.values() if isinstance(val, dict) else val if isinstance(val, (tuple, list)) else [val]):
            for b in (a if isinstance(a, (tuple, list)) else [a]):
                if isinstance(b, np.ndarray):
                    b.setflags(write=False)
        _CACHE[key] = val
    return _CACHE[key]


def _load(tag):
    return _cached(("npz", tag), lambda: dict(np.load(os.path.join(GOLDEN, "rq_%s.npz" % tag))))


def _module(rec, dev):
    """_rq_ref._module on copies: the cached record stays read-only"""
    return R._module({k: v.copy() for k, v in rec.items()}, dev)


def _golden_chain(name):
    case = CASES[name]
    g = _geom(case)
    rec = _load(case.tag)
    return _cached(("chain", name), lambda: R.chain(rec["x"], _books(rec, g.depth), rec["codes"].reshape(g.N, g.depth), g.rH, g.rW))


def _check_loss(what, got, ref, depth):
    """|got - ref| <= (depth + 2) 2^-24 |ref| (module docstring); the figure is printed before it is asserted"""
    got, ref = float(got), float(ref)
    dev = abs(got - ref) / abs(ref)
    print("rq loss deviation %s: %.9g vs %.9g, %.3g relative = %.3f of the bound %.3g"
          % (what, got, ref, dev, dev / ((depth + 2) * U), (depth + 2) * U))
    assert dev <= (depth + 2) * U, what


# ---- CPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", EVAL)
def test_new_goldens_match_the_restatement(oracle_mod, name):
    case = CASES[name]
    g = _geom(case)
    rec, emb = _load(case.tag), _load(case.tag + "_embed")
    assert tuple(rec["latent_shape"]) == case.latent and tuple(rec["code_shape"]) == case.code and rec["x"].shape[0] == case.B
    assert [int(k) for k in rec["n_embed"]] == case.n_embed and bool(rec["shared"]) == case.shared
    x = rec["x"]
    # the sign rules have something to bite on
    assert np.signbit(x.reshape(-1)[::7]).all() and not x.reshape(-1)[::7].any()
    assert np.signbit(rec["weight.0"][:-1][::5, ::3]).all() and not rec["weight.0"][:-1][::5, ::3].any()
    books = _books(rec, g.depth)
    codes, out, agg, loss = _restate(oracle_mod, x, books, g.rH, g.rW)
    assert np.array_equal(codes, rec["codes"])
    assert same_bits(out, rec["out"]) and same_bits(agg, rec["agg"])
    assert abs(loss - float(rec["loss"])) <= 1e-5 * abs(float(rec["loss"]))
    assert bool(rec["agg_equals_embed_code"]) and bool(rec["add_last_equals_embed_code"])
    ch = _golden_chain(name)
    assert same_bits(ch.out, rec["out"]) and same_bits(ch.agg, rec["agg"])
    assert abs(float(ch.loss) - float(rec["loss"])) <= 1e-5 * abs(float(rec["loss"]))
    assert len(ch.residuals) == g.depth - 1
    # the reference's embed reads the padding row too: K_t = n_embed + 1
    full = [rec["weight.0" if case.shared else "weight.%d" % i] for i in range(g.depth)]
    ci, geo = min(1, g.depth - 1), _geometry(g)
    assert same_bits(R.embed(full, rec["codes"], "sum", g.depth - 1, geo), emb["embed_code"])
    assert same_bits(R.embed(full, rec["codes"], "each", g.depth - 1, geo), emb["embed_code_with_depth"])
    assert same_bits(R.embed(full, rec["codes"], "select", ci, geo), emb["partial_select_%d" % ci])
    assert same_bits(R.embed(full, rec["codes"], "sum", ci, geo), emb["partial_add_%d" % ci])
    # -0 + -0 entries: SUM turns them into +0 (agg_0 = +0), SELECT keeps them
    sel0 = R.embed(full, rec["codes"], "select", 0, geo)
    sum0 = R.embed(full, rec["codes"], "sum", 0, geo)
    neg = np.signbit(sel0) & (sel0 == 0)
    assert neg.any() and not np.signbit(sum0[neg]).any()


def _ceil256(b):
    return (b + 255) // 256 * 256


def _blocks(N, D):
    return min(2048, -(-N * D // 1024))


def test_case_table_reaches_what_it_claims():
    L = _lib.lib
    src = open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "rq.hip")).read()
    flat = re.sub(r"\s+", " ", src)
    hint = " -- rq.hip changed its block count or its vector-width rule: rebuild the case table of tests/test_rq_shapes.py for it"
    for line in ("const long b = (N * D + 1023) / 1024;", "return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));",
                 "const bool v4 = Dl % 4 == 0 && al16(x) && al16(r_in) && al16(E) && al16(out);",
                 "if (Dl % 4 == 0 && al16(g_out) && al16(g_x))", "bool v4 = Dl % 4 == 0 && al16(out);",
                 "for (int k = threadIdx.x; k < nparts; k += 256)",
                 "for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < chunks; q += gridDim.x * 256u)"):
        assert line in flat, line + hint
    assert _lib.RQ_MAX_DEPTH == 16
    reached = set()
    for name, case in CASES.items():
        g = _geom(case)
        N, D, depth = g.N, g.D, g.depth
        P = _blocks(N, D)
        row = _ceil256(N * D * 4)
        # the loss partials come first: the first residual slot starts behind depth x P doubles
        if depth >= 2:
            assert L.dvq_rq_residual_offset(N, D, depth, 1) == _ceil256(depth * P * 8), name
        else:
            assert L.dvq_rq_residual_offset(N, D, depth, 1) == 0, name
        if depth >= 3:
            assert L.dvq_rq_residual_offset(N, D, depth, 2) == _ceil256(depth * P * 8) + row, name
        for i in range(3, depth):                                 # the two slots alternate
            assert L.dvq_rq_residual_offset(N, D, depth, i) == L.dvq_rq_residual_offset(N, D, depth, i - 2), name
        # [loss partials depth x P doubles][residual slot 0][residual slot 1][agg][s (want_grad)], every section 256-byte aligned
        for d in (1, 2, 3, depth):
            for want_grad in (0, 1):
                want = _ceil256(d * P * 8) + (min(d - 1, 2) + (1 if d > 1 else 0) + want_grad) * row
                assert L.dvq_rq_workspace_bytes(N, D, d, want_grad) == want, (name, d, want_grad)
        claims = {"vw4" if g.Dl % 4 == 0 else "vw1"}
        if (N * D) % 1024:
            claims.add("ragged")
        if P > 256:
            claims.add("partials>256")
        if P == 2048 and N * D // 4 > 2048 * 256:
            claims.add("capped")
        if depth in (1, 2, 16):
            claims.add("depth%d" % depth)
        assert case.claims <= claims, (name, case.claims - claims)
        reached |= case.claims
    assert reached == {"vw1", "vw4", "ragged", "partials>256", "capped", "depth1", "depth2", "depth16"}
    g1, g2 = _geom(CASES["L1"]), _geom(CASES["L2"])
    assert _blocks(g1.N, g1.D) == 300 and g1.N * g1.D == 307200
    assert g2.N * g2.D // 4 == 614400 and _blocks(g2.N, g2.D) * 256 == 524288
    for name in ("G1", "G2", "G5", "T1", "S2", "L1", "L2"):       # a swap of rH / rW or of h / w shows only where they differ
        g = _geom(CASES[name])
        assert g.rH != g.rW and (g.h != g.w or name == "L1"), name
    assert _geom(CASES["G3"]).h != _geom(CASES["G3"]).w


# ---- GPU, module level ------------------------------------------------------------------------------------------------------

def _t(dev):
    return lambda a: torch.tensor(np.ascontiguousarray(a), device=dev)            # a copy: the cached inputs are read-only


def _off_alignment(a):
    """a copy of the tensor that starts one float behind a 16-byte boundary"""
    buf = torch.empty(a.numel() + 1, dtype=a.dtype, device=a.device)
    v = buf[1:].view(a.shape)
    v.copy_(a)
    assert v.data_ptr() % 16 == 4
    return v


def _poison(nbytes, dev):
    return torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=dev)


def _poison_f32(shape, dev):
    return _poison(int(np.prod(shape)) * 4, dev).view(torch.float32).view(shape)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [_lib.MODE_FILTER, _lib.MODE_EXACT])
@pytest.mark.parametrize("name", EVAL)
def test_eval_ragged_golden(dev, name, mode):
    case = CASES[name]
    g = _geom(case)
    rec, emb = _load(case.tag), _load(case.tag + "_embed")
    rq = _module(rec, dev).eval()
    rq.assign_mode = mode
    t = _t(dev)
    x = t(rec["x"])
    # a stale workspace under the key _rq_forward looks up: every byte 0xFF, so whatever a kernel read of it would be a NaN
    key = (x.device, _lib.stream_ptr(x.device), g.N, g.D, g.depth)
    stale = rq._ws[key] = _poison(_lib.lib.dvq_rq_workspace_bytes(g.N, g.D, g.depth, 0), dev)
    with torch.no_grad():
        out, loss, codes = rq(x)
        assert len(rq._ws) == 1 and rq._ws[key] is stale
        assert torch.equal(rq.get_codes(x), codes)
    assert np.array_equal(codes.cpu().numpy(), rec["codes"])
    assert same_bits(out.cpu().numpy(), rec["out"])
    assert loss.dim() == 0 and abs(float(loss) - float(rec["loss"])) <= 1e-5 * abs(float(rec["loss"]))
    _check_loss("%s mode %d" % (name, mode), loss, _golden_chain(name).loss, g.depth)
    d, ci = g.depth, min(1, g.depth - 1)
    assert same_bits(rq.embed_code(codes).cpu().numpy(), emb["embed_code"])
    assert same_bits(rq.embed_code(codes).cpu().numpy(), rec["agg"])
    assert same_bits(rq.embed_partial_code(codes, d - 1, "add").cpu().numpy(), emb["embed_code"])
    assert same_bits(rq.embed_partial_code(codes, ci, "add").cpu().numpy(), emb["partial_add_%d" % ci])
    assert same_bits(rq.embed_partial_code(codes, ci, "select").cpu().numpy(), emb["partial_select_%d" % ci])
    ed, none = rq.embed_code_with_depth(codes, to_latent_shape=True)
    assert none is None and same_bits(ed.cpu().numpy(), emb["embed_code_with_depth"])
    ec, _ = rq.embed_code_with_depth(codes)
    books = _books(rec, d)
    assert same_bits(ec.cpu().numpy(), np.stack([books[i][rec["codes"][..., i]] for i in range(d)], -2))
    # one float off 16-byte alignment (the 4-byte kernels), over a workspace made stale again: the same bits
    stale.fill_(0xFF)
    xm = _off_alignment(x)
    with torch.no_grad():
        outm, lossm, codesm = rq(xm)
        assert rq._ws[key] is stale
    assert torch.equal(codesm, codes) and same_bits(outm.cpu().numpy(), rec["out"])
    assert same_bits(lossm.reshape(1).cpu().numpy(), loss.reshape(1).cpu().numpy())


def _randperm_reversed(n, *a, **kw):
    return torch.arange(n - 1, -1, -1, device=kw.get("device"))


@pytest.mark.gpu
def test_train_ragged_golden(dev, oracle_mod, monkeypatch):
    case = CASES["T1"]
    g = _geom(case)
    rec = _load(case.tag)
    rq = _module(rec, dev).train()
    t = _t(dev)
    x = t(rec["x"]).requires_grad_(True)
    # depth i gathers from the codebook as the EMA update of depth i - 1 left it: keep each depth's rows for the restatement
    cb = rq.codebooks[0]
    used, update = [], cb._update_buffers

    def recording(vectors, idxs, *a, **kw):
        used.append(cb.weight.detach()[:-1].cpu().numpy().copy())
        return update(vectors, idxs, *a, **kw)

    monkeypatch.setattr(cb, "_update_buffers", recording)
    monkeypatch.setattr(torch, "randperm", _randperm_reversed)
    out, loss, codes = rq(x)
    monkeypatch.undo()
    ((out * t(rec["R"])).sum() + 3.0 * loss).backward()
    assert np.array_equal(codes.cpu().numpy(), rec["codes"])
    # depth i + 1 gathers from the codebook the EMA update of depth i wrote, whose cluster sums are tolerance-level (summation order)
    assert np.abs(out.detach().cpu().numpy() - rec["out"]).max() <= 1e-5 * np.abs(rec["out"]).max()
    assert abs(float(loss.detach()) - float(rec["loss"])) <= 1e-5 * abs(float(rec["loss"]))
    gx = x.grad.cpu().numpy()
    assert np.abs(gx - rec["grad_x"]).max() <= 1e-6 * max(1.0, np.abs(rec["grad_x"]).max())
    for name in ("weight", "cluster_size_ema", "embed_ema"):
        got, ref = getattr(cb, name).detach().cpu().numpy(), rec["after.%s.0" % name]
        assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), name
    # given the rows each depth gathered and the codes of the run, out and x.grad are the header's recipe bit for bit
    assert len(used) == g.depth and not np.array_equal(used[0], used[1])
    ch = R.chain(rec["x"], used, codes.cpu().numpy().reshape(g.N, g.depth), g.rH, g.rW)
    assert same_bits(out.detach().cpu().numpy(), ch.out)
    _check_loss("T1 training step", loss.detach(), ch.loss, g.depth)
    assert same_bits(gx, R.grad(rec["R"], 3.0, ch.s, g.N, g.D, g.depth, _geometry(g)))
    # the next eval forward searches the updated codebooks: the restatement on OUR updated weights
    rq.eval()
    with torch.no_grad():
        _, _, codes2 = rq(x.detach())
    books = [cb.weight.detach().cpu().numpy()[:-1]] * g.depth
    ref_codes, _, _, _ = _restate(oracle_mod, rec["x"], books, g.rH, g.rW)
    assert np.array_equal(codes2.cpu().numpy(), ref_codes)


def _fresh_latents(case, E, seed):
    g = _geom(case)
    z = synth.z_tokens(E, g.B, g.h, g.w, seed)
    return _to_latent(np.ascontiguousarray(z.transpose(0, 2, 3, 1)), g.rH, g.rW, g.Dl)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("G1", "G2", "G3"))
def test_backward_parts_ragged(dev, name):
    case = CASES[name]
    g = _geom(case)
    rec = _load(case.tag)
    rq = _module(rec, dev).eval()
    books = _books(rec, g.depth)
    x0 = _fresh_latents(case, books[0], 3101 + EVAL.index(name))
    Rn = synth.normal(3111 + EVAL.index(name), x0.shape)
    t = _t(dev)
    runs = []
    for form in ("out", "loss", "both"):
        x = t(x0).requires_grad_(True)
        out, loss, codes = rq(x)
        {"out": lambda: out.sum(), "loss": lambda: loss, "both": lambda: (out * t(Rn)).sum() + 3.0 * loss}[form]().backward()
        runs.append((x.grad.cpu().numpy(), codes.cpu().numpy(), out.detach().cpu().numpy(), loss.detach()))
    assert np.array_equal(runs[0][1], runs[1][1]) and np.array_equal(runs[0][1], runs[2][1])
    ch = R.chain(x0, books, runs[0][1].reshape(g.N, g.depth), g.rH, g.rW)
    geo = _geometry(g)
    for r in runs:
        assert same_bits(r[2], ch.out)
    _check_loss("%s backward parts" % name, runs[0][3], ch.loss, g.depth)
    assert same_bits(runs[0][0], np.ones_like(x0))
    assert same_bits(runs[0][0], R.grad(np.ones_like(x0), 0.0, ch.s, g.N, g.D, g.depth, geo))
    assert same_bits(runs[1][0], R.grad(None, 1.0, ch.s, g.N, g.D, g.depth, geo))
    assert same_bits(runs[2][0], R.grad(Rn, 3.0, ch.s, g.N, g.D, g.depth, geo))
    assert np.abs(runs[1][0]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("S2", "G5"))
def test_soft_codes_ragged(dev, name):
    from dynamicvectorquantization_amd.quantize import soft_assign
    case = CASES[name]
    g = _geom(case)
    if case.tag is None:
        rq = RQBottleneck(case.latent, case.code, case.n_embed).to(dev).eval()
        for i, cb in enumerate(rq.codebooks):
            Ei = synth.codebook_trained(cb.n_embed, g.D, seed=3201 + i) * np.float32(1.0 if i == 0 else 0.3)
            cb.weight.data[:-1].copy_(torch.from_numpy(Ei))
            cb.invalidate_codebook_cache()
        x = _t(dev)(_fresh_latents(case, rq.codebooks[0].weight.detach()[:-1].cpu().numpy(), 3211))
    else:
        rec = _load(case.tag)
        rq = _module(rec, dev).eval()
        x = _t(dev)(rec["x"])
    K = case.n_embed[0]
    soft, hard = rq.get_soft_codes(x, temp=8.0)
    assert soft.shape == (g.B, g.h, g.w, g.depth, K) and torch.equal(hard, rq.get_codes(x))
    if case.tag is not None:
        assert np.array_equal(hard.cpu().numpy(), _load(case.tag)["codes"])
    ws = next(iter(rq._ws.values()))
    for i in range(g.depth):
        if i == 0:
            r = rq.to_code_shape(x).reshape(g.N, g.D)
            assert same_bits(r.cpu().numpy(), _to_code(x.cpu().numpy(), g.rH, g.rW).reshape(g.N, g.D))
        else:
            off = _lib.lib.dvq_rq_residual_offset(g.N, g.D, g.depth, i)
            assert off > 0
            r = ws[off:off + g.N * g.D * 4].view(torch.float32).view(g.N, g.D)
        cb = rq.codebooks[i]
        s_i, c_i, _ = soft_assign(r.clone(), cb.weight[:-1], cb._prep, 8.0)
        assert torch.equal(soft[..., i, :].reshape(g.N, K), s_i) and torch.equal(hard[..., i].reshape(g.N), c_i)
    torch.manual_seed(7)
    s1, c1 = rq.get_soft_codes(x, temp=8.0, stochastic=True)
    torch.manual_seed(7)
    s2, c2 = rq.get_soft_codes(x, temp=8.0, stochastic=True)
    assert torch.equal(c1, c2) and torch.equal(s1, s2) and int(c1.min()) >= 0 and int(c1.max()) < K
    assert torch.equal(s1[..., 0, :], soft[..., 0, :])               # depth 0 sees the same residual either way


@pytest.mark.gpu
def test_empty_batch(dev):
    case = CASES["G2"]
    (H, W, Dl), (h, w, depth) = case.latent, case.code
    rq = _module(_load(case.tag), dev).eval()
    x = torch.zeros((0, H, W, Dl), device=dev)
    with torch.no_grad():
        out, loss, codes = rq(x)
        assert out.shape == (0, H, W, Dl) and codes.shape == (0, h, w, depth) and codes.dtype == torch.int64
        assert loss.dim() == 0 and bool(torch.isnan(loss))
        assert rq.get_codes(x).shape == (0, h, w, depth)
        assert rq.embed_code(codes).shape == (0, H, W, Dl)
        assert rq.embed_partial_code(codes, 1, "select").shape == (0, H, W, Dl)
        assert rq.embed_code_with_depth(codes, to_latent_shape=True)[0].shape == (0, H, W, depth, Dl)
        soft, sc = rq.get_soft_codes(x)
        assert soft.shape[:4] == (0, h, w, depth) and sc.shape == (0, h, w, depth)
    xg = torch.zeros((0, H, W, Dl), device=dev, requires_grad=True)
    out, loss, codes = rq(xg)
    assert out.shape == (0, H, W, Dl) and codes.shape == (0, h, w, depth) and bool(torch.isnan(loss))
    (out.sum() + loss).backward()
    torch.cuda.synchronize()
    assert xg.grad is not None and xg.grad.shape == (0, H, W, Dl)


# ---- GPU, ABI level with given codes ----------------------------------------------------------------------------------------

def _given(name):
    """x, the codebooks (the K_i rows a step may gather) and codes [N, depth] drawn without a search; -0.0 planted as in the goldens"""
    case = CASES[name]
    g = _geom(case)

    def make():
        seed = 3301 + 20 * GIVEN.index(name)
        x = synth.normal(seed, (g.B, g.h * g.rH, g.w * g.rW, g.Dl))
        x.reshape(-1)[::7] = -0.0
        books = []
        for i, K in enumerate(case.n_embed):
            if case.shared and i:
                books.append(books[0])
                continue
            E = synth.codebook_trained(K, g.D, seed=seed + 1 + i)
            E[::5, ::3] = -0.0
            books.append(E)
        codes = np.stack([synth.randint(seed + 17, (g.N,), K, offset=i * g.N) for i, K in enumerate(case.n_embed)], 1)
        return {"x": x, "books": books, "codes": codes}

    return _cached(("given", name), make)


def _given_chain(name):
    g, inp = _geom(CASES[name]), _given(name)
    return _cached(("given-chain", name), lambda: R.chain(inp["x"], inp["books"], inp["codes"], g.rH, g.rW))


class _AbiRun:
    """dvq_rq_step_f32 for i = 0 .. depth-1 by hand into a want_grad workspace filled with 0xFF, then dvq_rq_loss_f32"""

    def __init__(self, dev, g, x, books, codes, misalign=False):
        L = _lib.checked
        t = _t(dev)
        self.dev, self.g, self.stream = dev, g, _lib.stream_ptr(dev)
        self.nbytes = L.dvq_rq_workspace_bytes(g.N, g.D, g.depth, 1)
        assert self.nbytes > 0
        self.ws = _poison(self.nbytes, dev)
        assert self.ws.data_ptr() % 256 == 0
        xd = t(x)
        self.x = _off_alignment(xd) if misalign else xd
        self.out = _poison_f32(x.shape, dev)
        if misalign:
            self.out = _off_alignment(self.out)
        r = self.x if g.rH == 1 and g.rW == 1 else t(_to_code(x, g.rH, g.rW))
        self.books = [t(E) for E in books]
        self.codes_out = torch.full((g.N, g.depth), -7, dtype=torch.int64, device=dev)
        self.residuals = []
        self.out_before_last = None
        for i in range(g.depth):
            if i == g.depth - 1:
                self.out_before_last = self.out.cpu().numpy()
            c = t(codes[:, i])
            L.dvq_rq_step_f32(self.x.data_ptr(), r.data_ptr(), self.books[i].data_ptr(), int(books[i].shape[0]), c.data_ptr(),
                              g.B, g.h, g.w, g.rH, g.rW, g.Dl, g.D, i, g.depth, 1, self.codes_out.data_ptr(), self.out.data_ptr(),
                              self.ws.data_ptr(), self.nbytes, self.stream)
            if i + 1 < g.depth:
                off = L.dvq_rq_residual_offset(g.N, g.D, g.depth, i + 1)
                assert off > 0 and off + g.N * g.D * 4 <= self.nbytes
                r = self.ws[off:off + g.N * g.D * 4].view(torch.float32).view(g.N, g.D)
                self.residuals.append(r.cpu().numpy())
        loss = _poison_f32((1,), dev)
        L.dvq_rq_loss_f32(g.N, g.D, g.depth, self.ws.data_ptr(), self.nbytes, loss.data_ptr(), self.stream)
        self.loss = loss.cpu().numpy()
        self.out_np = self.out.cpu().numpy()
        self.codes_np = self.codes_out.cpu().numpy()

    def backward(self, g_out, g_loss, misalign=False):
        g, t = self.g, _t(self.dev)
        go = None if g_out is None else t(g_out)
        gl = None if g_loss is None else t(np.array([g_loss], np.float32))
        gx = _poison_f32(self.out.shape, self.dev)
        if misalign:
            gx = _off_alignment(gx)
            go = None if go is None else _off_alignment(go)
        _lib.checked.dvq_rq_backward_f32(_lib.ptr(go) or None, _lib.ptr(gl) or None, g.B, g.h, g.w, g.rH, g.rW, g.Dl, g.D, g.depth,
                                         self.ws.data_ptr(), self.nbytes, gx.data_ptr(), self.stream)
        return gx.cpu().numpy()


def _abi_embed(dev, books, codes, mode, j, geometry, dbooks=None):
    """dvq_rq_embed_code_f32 into an output filled with 0xFF; books[t] = all K_t rows a code may address"""
    B, h, w, rH, rW, Dl = geometry
    depth = len(books)
    t = _t(dev)
    dbooks = [t(E) for E in books] if dbooks is None else dbooks
    ptrs = (ctypes.c_void_p * depth)(*[E.data_ptr() for E in dbooks])
    ks = (ctypes.c_int * depth)(*[int(E.shape[0]) for E in books])
    shape = (B, h * rH, w * rW, j + 1, Dl) if mode == "each" else (B, h * rH, w * rW, Dl)
    out = _poison_f32(shape, dev)
    c = t(codes)
    _lib.checked.dvq_rq_embed_code_f32(ptrs, ks, depth, c.data_ptr(), B, h, w, rH, rW, Dl, rH * rW * Dl,
                                       {"sum": 0, "select": 1, "each": 2}[mode], j, out.data_ptr(), _lib.stream_ptr(dev))
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", GIVEN)
def test_step_chain_given_codes(dev, name):
    g, inp, ch = _geom(CASES[name]), _given(name), _given_chain(name)
    x, books, codes = inp["x"], inp["books"], inp["codes"]
    geo = _geometry(g)
    run = _AbiRun(dev, g, x, books, codes)
    assert len(run.residuals) == len(ch.residuals) == g.depth - 1
    for i, (got, ref) in enumerate(zip(run.residuals, ch.residuals)):
        assert same_bits(got, ref), "r_%d" % (i + 1)
    assert (run.out_before_last.view(np.uint32) == 0xFFFFFFFF).all()          # out is written on the last depth only
    assert same_bits(run.out_np, ch.out)
    assert np.array_equal(run.codes_np, codes)
    _check_loss("%s given codes" % name, run.loss[0], ch.loss, g.depth)
    # the backward in the four null / non-null combinations
    g_out = synth.normal(3390 + GIVEN.index(name), x.shape)
    for go, gl in ((None, None), (g_out, None), (None, 3.0), (g_out, 3.0)):
        got = run.backward(go, gl)
        assert same_bits(got, R.grad(go, gl, ch.s, g.N, g.D, g.depth, geo)), (go is None, gl)
    assert same_bits(run.backward(g_out, 3.0, misalign=True), R.grad(g_out, 3.0, ch.s, g.N, g.D, g.depth, geo))
    # the embed: three modes, j = 0 and j = depth - 1, latent layout and its code-layout form
    for layout in (geo, (g.B, g.h, g.w, 1, 1, g.D)):
        for mode in ("sum", "select", "each"):
            for j in sorted({0, g.depth - 1}):
                got = _abi_embed(dev, books, codes, mode, j, layout, run.books)
                assert same_bits(got, R.embed(books, codes, mode, j, layout)), (layout, mode, j)
    # a second full chain: the same bits; and with x and out one float off 16-byte alignment
    again = _AbiRun(dev, g, x, books, codes)
    assert same_bits(again.loss, run.loss) and same_bits(again.out_np, run.out_np)
    off = _AbiRun(dev, g, x, books, codes, misalign=True)
    for i, (got, ref) in enumerate(zip(off.residuals, run.residuals)):
        assert same_bits(got, ref), "r_%d off alignment" % (i + 1)
    assert same_bits(off.out_np, run.out_np) and same_bits(off.loss, run.loss) and np.array_equal(off.codes_np, codes)


def _same_where_not_nan(got, ref):
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(got), nan)) and same_bits(np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), ref))


@pytest.mark.gpu
def test_codes_out_of_range_give_nan_rows(dev):
    case = CASES["G2"]
    g, inp = _geom(case), _given("G2")
    x, books = inp["x"], inp["books"]
    geo = _geometry(g)
    K0, K1 = case.n_embed
    codes = inp["codes"].copy()
    bad = np.array([0, 37, g.N - 1])
    codes[bad, 0] = [-1, K0, 2 ** 40]
    good = np.setdiff1d(np.arange(g.N), bad)
    ch = R.chain(x, books, codes, g.rH, g.rW)
    run = _AbiRun(dev, g, x, books, codes)
    r1, outc = run.residuals[0], _to_code(run.out_np, g.rH, g.rW).reshape(g.N, g.D)
    assert np.isnan(r1[bad]).all() and np.isnan(outc[bad]).all()
    assert same_bits(r1[good], ch.residuals[0][good])
    assert same_bits(outc[good], _to_code(ch.out, g.rH, g.rW).reshape(g.N, g.D)[good]) and not np.isnan(outc[good]).any()
    assert np.array_equal(run.codes_np, codes)                  # recorded as given
    assert np.isnan(run.loss[0]) and np.isnan(ch.loss)
    # the embed with K_t = n_embed + 1: the padding row is a row like any other, the codes around it are not
    full = [np.concatenate([E, synth.normal(3401 + i, (1, g.D))]) for i, E in enumerate(books)]
    codes = inp["codes"].copy()
    codes[1, 0], codes[2, 1], codes[3, 0], codes[4, 1], codes[5, 0] = K0, K1 + 1, -1, K1, K0 + 1
    nan_at = {0: [3, 5], 1: [2]}                                 # depth -> tokens whose code of that depth is out of range
    code_rows = lambda a: _to_code(a, g.rH, g.rW).reshape(g.N, g.D)
    for mode, j in (("sum", 0), ("sum", 1), ("select", 0), ("select", 1), ("each", 1)):
        got = _abi_embed(dev, full, codes, mode, j, geo)
        assert _same_where_not_nan(got, R.embed(full, codes, mode, j, geo)), (mode, j)
        if mode == "each":
            rows = [code_rows(np.ascontiguousarray(got[..., t, :])) for t in range(j + 1)]
            for t in range(j + 1):
                nan_rows = np.isnan(rows[t]).all(1)
                assert np.array_equal(np.flatnonzero(nan_rows), nan_at[t]) and not np.isnan(rows[t][~nan_rows]).any()
            assert same_bits(rows[0][1], full[0][K0]) and same_bits(rows[1][4], full[1][K1])
            continue
        rows = code_rows(got)
        want_nan = sorted(nan_at[j] if mode == "select" else sum((nan_at[t] for t in range(j + 1)), []))
        nan_rows = np.isnan(rows).all(1)
        assert np.array_equal(np.flatnonzero(nan_rows), want_nan) and not np.isnan(rows[~nan_rows]).any()
        if mode == "select":
            pad_token, pad_row = (1, full[0][K0]) if j == 0 else (4, full[1][K1])
            assert same_bits(rows[pad_token], pad_row)
