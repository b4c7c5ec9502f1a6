"""The fused orthogonal loss (csrc/ortho_loss.hip) away from the shapes of its golden fixtures, which all have h = 1 and
T = ceil(n / 32) in 3, 4 and 32: several heads, a single partial tile, a ragged last forward workgroup over more than one row
chunk, backward slice counts with a short last slice, fewer slices than first estimated, and one slice.  tests/test_lucid.py holds
the fixtures; the float64 expression and the restatement of the launch geometry are in tests/_lucid_ref.py.

Inputs: head i of t [h, n, d] = synth.codebook_trained(n, d, seed + i) scaled by 1 + i / 4 (mod 2); in head min(1, h - 1) of every
multi-head case row 7 is zero and row n - 2 (another tile) is a copy of row 3.

  case  h    n     d    seed  what it reaches (OrthoGeom of _lucid_ref.ortho_geometry)
  S     1    5     64   7801  T = 1: one partial tile, S = 1
  I     1    33    256  7811  T = 2: two idle waves in the only forward workgroup; S = 2
  R     1    289   64   7821  T = 10: forward grid 3 x 2, two idle waves in the last workgroup of each row chunk; S = 5 where the
                              first estimate was 8
  H     3    100   64   7831  heads; S = 4
  L     2    1056  128  7841  T = 33: forward grid 9 x 5; S = 7, the last slice 3 tiles of tper = 5
  M     200  96    64   7851  S = 1, the many-heads end of dvq_ortho_backward_slices

`test_case_table_reaches_what_it_claims` derives the last column from the restated geometry and checks the slice count against
dvq_ortho_loss_workspace_bytes, without a device.

Bounds (those of tests/test_lucid.py's test_orthogonal_loss): the loss within 1e-5 relative of float64 (mean over the heads); two
runs the same bits; the gradient's max-abs error against float64 (each head's gradient / h, times the upstream factor), normalised
by max |g64|, at most 4 x that of the reference's own fp32 CPU gradient (`_orthogonal_loss_torch` on CPU tensors, then backward),
measured at run time.  Row permutation: permuting one head's rows permutes that head's gradient rows, leaves the other heads' bits
alone and moves the loss by at most 1e-6 relative (the summation order changes).

What the cases see.  Two mistakes that stay in bounds were tried on a scratch build.  A backward slice's partial G stored at
[head][slice] where the combine kernel reads [slice][head]: the gradient bound fails in H and L (and the tests built on H); the
h = 1 cases and M (S = 1) cannot see it.  The forward partial of a workgroup indexed with gridDim.y in place of gridDim.x: only L
fails (the loss, and its bits between two runs); grids of one workgroup per head are unchanged by it, and in R the one workgroup
that collides lies wholly below the diagonal and contributes nothing."""
import collections
import os
import re

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib, synth
from tests import _lucid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UPSTREAM = 1.5

Case = collections.namedtuple("Case", "h n d seed claims")
CASES = {
    "S": Case(1, 5, 64, 7801, {"single_tile"}),
    "I": Case(1, 33, 256, 7811, {"idle_waves"}),
    "R": Case(1, 289, 64, 7821, {"idle_waves", "row_chunks", "ragged_forward", "reduced_S"}),
    "H": Case(3, 100, 64, 7831, {"heads"}),
    "L": Case(2, 1056, 128, 7841, {"heads", "idle_waves", "row_chunks", "ragged_forward", "short_last_slice", "reduced_S"}),
    "M": Case(200, 96, 64, 7851, {"heads", "idle_waves", "one_slice"}),
}
NAMES = tuple(CASES)

_CACHE = {}


def _planted(c):
    """(head, zero row, copied row, its source) of a multi-head case"""
    return min(1, c.h - 1), 7, c.n - 2, 3


def _inputs(name):
    """t, the float64 loss and gradient, and the reference's own fp32 CPU loss and gradient error: computed once, read-only"""
    if name not in _CACHE:
        c = CASES[name]
        t = np.stack([synth.codebook_trained(c.n, c.d, seed=c.seed + i) * np.float32(1.0 + (i % 2) / 4.0) for i in range(c.h)])
        if c.h > 1:
            head, zero, copy, src = _planted(c)
            t[head, zero] = 0.0
            t[head, copy] = t[head, src]
        loss64, g64 = R.ortho64_heads(t)
        from dynamicvectorquantization_amd.lucid import _orthogonal_loss_torch
        tc = torch.tensor(t, requires_grad=True)
        loss32 = _orthogonal_loss_torch(tc)
        (loss32 * UPSTREAM).backward()
        err32 = float(np.abs(tc.grad.numpy().astype(np.float64) - UPSTREAM * g64).max() / np.abs(UPSTREAM * g64).max())
        val = {"t": t, "loss64": loss64, "g64": g64, "loss32": float(loss32.detach()), "err32": err32}
        for a in val.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE[name] = val
    return _CACHE[name]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- CPU --------------------------------------------------------------------------------------------------------------------

def test_case_table_reaches_what_it_claims():
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "ortho_loss.hip")).read())
    hint = " -- ortho_loss.hip changed its launch geometry: rebuild the case table of tests/test_ortho_shapes.py for it"
    for line in ("#define OL_ROWCHUNK 8", "*gx = (unsigned)((T + 3) / 4);", "*gy = (unsigned)((T + OL_ROWCHUNK - 1) / OL_ROWCHUNK);",
                 "int s = (int)(1024 / (waves < 1 ? 1 : waves));", "s = s < 1 ? 1 : (s > 8 ? 8 : s);", "s = s > T ? T : s;",
                 "*tper = (T + s - 1) / s;", "*S = (T + *tper - 1) / *tper;",
                 "dim3((unsigned)((T + 3) / 4), (unsigned)h, (unsigned)S)", "dim3(gx, gy, (unsigned)h)"):
        assert line in src, line + hint
    reached = set()
    for name, c in CASES.items():
        g = R.ortho_geometry(c.h, c.n)
        # the backward partials are the larger section at every shape of the table: the byte count pins S
        assert g.S * c.h * c.n * c.d * 4 > g.gx * g.gy * c.h * 8
        assert _lib.lib.dvq_ortho_loss_workspace_bytes(c.h, c.n, c.d) == R.ortho_workspace_bytes(c.h, c.n, c.d), name
        assert (g.S - 1) * g.tper < g.T <= g.S * g.tper and 1 <= g.last <= g.tper
        claims = set()
        if g.T == 1 and c.n % 32:
            claims.add("single_tile")
        if g.idle:
            claims.add("idle_waves")                              # the last forward workgroup has waves without a column tile
        if g.gy > 1:
            claims.add("row_chunks")
        if g.idle and g.gy > 1 and g.gx > 1:
            claims.add("ragged_forward")
        if g.last < g.tper:
            claims.add("short_last_slice")
        if g.S < g.s0:
            claims.add("reduced_S")
        if g.S == 1 and c.h > 1:
            claims.add("one_slice")
        if c.h > 1:
            claims.add("heads")
        assert c.claims <= claims, (name, c.claims - claims)
        reached |= c.claims
    assert reached == {"single_tile", "idle_waves", "row_chunks", "ragged_forward", "short_last_slice", "reduced_S", "one_slice", "heads"}
    G = {name: R.ortho_geometry(c.h, c.n) for name, c in CASES.items()}
    assert G["S"][:4] == (1, 1, 1, 3) and G["S"].S == 1
    assert G["I"].T == 2 and G["I"].idle == 2 and (G["I"].gx, G["I"].gy) == (1, 1) and G["I"].S == 2
    assert G["R"].T == 10 and (G["R"].gx, G["R"].gy) == (3, 2) and G["R"].idle == 2 and (G["R"].s0, G["R"].S) == (8, 5)
    assert G["H"].S == 4
    assert G["L"].T == 33 and (G["L"].gx, G["L"].gy) == (9, 5) and (G["L"].S, G["L"].tper, G["L"].last) == (7, 5, 3)
    assert G["M"].S == 1 and G["M"].tper == G["M"].T == 3
    # the tile counts of the golden fixtures, for the record: none of the above
    assert [R.ortho_geometry(1, n).T for n in (96, 100, 1024)] == [3, 4, 32]


@pytest.mark.parametrize("name", NAMES)
def test_reference_own_error(name):
    """the float64 restatement per head against torch's float64 autograd, and the yardstick: the reference's fp32 CPU gradient"""
    from dynamicvectorquantization_amd.lucid import _orthogonal_loss_torch
    c, inp = CASES[name], _inputs(name)
    print("%s: reference fp32 CPU loss %.3g relative off float64, gradient error %.3g" %
          (name, abs(inp["loss32"] - inp["loss64"]) / inp["loss64"], inp["err32"]))
    assert abs(inp["loss32"] - inp["loss64"]) <= 1e-5 * inp["loss64"]
    assert 0.0 < inp["err32"] < 1e-4                                # a yardstick of zero would make the factor-4 rule vacuous
    t = torch.tensor(inp["t"], dtype=torch.float64, requires_grad=True)
    loss = _orthogonal_loss_torch(t)
    loss.backward()
    assert abs(float(loss.detach()) - inp["loss64"]) <= 1e-12 * inp["loss64"]
    assert np.abs(t.grad.numpy() - inp["g64"]).max() <= 1e-12 * np.abs(inp["g64"]).max()
    if c.h > 1:
        head, zero, copy, src = _planted(c)
        assert not inp["t"][head, zero].any() and np.array_equal(inp["t"][head, copy], inp["t"][head, src])
        assert not inp["g64"][head, zero].any() and copy // 32 != src // 32


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _t(a, dev):
    return torch.tensor(np.ascontiguousarray(a), device=dev)


def _fused(loss):
    assert type(loss.grad_fn).__name__.startswith("_OrthogonalLoss")              # the kernels, not the torch expression
    return loss


def _run(t_np, dev, upstream=UPSTREAM):
    from dynamicvectorquantization_amd import lucid
    t = _t(t_np, dev).requires_grad_(True)
    loss = _fused(lucid.orthogonal_loss_fn(t))
    (loss * upstream).backward()
    assert t.grad.shape == t.shape
    return loss.detach().cpu().numpy().reshape(1).copy(), t.grad.cpu().numpy().copy()


def _check(what, loss, grad, inp, g64=None):
    """the two bounds of the module docstring; both figures are printed before they are asserted"""
    g64 = UPSTREAM * (inp["g64"] if g64 is None else g64)
    err = float(np.abs(grad.astype(np.float64) - g64).max() / np.abs(g64).max())
    dev = abs(float(loss[0]) - inp["loss64"]) / inp["loss64"]
    print("%s: loss %.9g (float64 %.9g, %.3g relative)  gradient error %.3g, the reference's fp32 %.3g" %
          (what, float(loss[0]), inp["loss64"], dev, err, inp["err32"]))
    assert dev <= 1e-5, what
    assert np.isfinite(grad).all() and err <= 4.0 * inp["err32"], what


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_case(name, dev):
    c, inp = CASES[name], _inputs(name)
    one, two = _run(inp["t"], dev), _run(inp["t"], dev)
    assert np.array_equal(_bits(one[0]), _bits(two[0])) and np.array_equal(_bits(one[1]), _bits(two[1]))
    _check("%s (h=%d n=%d d=%d)" % (name, c.h, c.n, c.d), one[0], one[1], inp)
    if c.h > 1:                                                    # each head against its own largest gradient element too
        g64 = UPSTREAM * inp["g64"]
        per_head = np.abs(one[1].astype(np.float64) - g64).max(axis=(1, 2)) / np.abs(g64).max(axis=(1, 2))
        print("%s: largest per-head gradient error %.3g" % (name, per_head.max()))
        head, zero, _, _ = _planted(c)
        assert not one[1][head, zero].any()                        # the zero row: c^ = 0, G = 0
    if c.h == 1:
        from dynamicvectorquantization_amd import lucid
        flat = _fused(lucid.orthogonal_loss_fn(_t(inp["t"][0], dev).requires_grad_(True)))      # [n, d]: h = 1
        assert np.array_equal(_bits(flat.detach().cpu().numpy().reshape(1)), _bits(one[0]))


@pytest.mark.gpu
def test_upstream_gradient_is_a_tensor_expression(dev):
    from dynamicvectorquantization_amd import lucid
    inp = _inputs("H")
    t = _t(inp["t"], dev).requires_grad_(True)
    k = torch.tensor([0.25, 1.25], device=dev, requires_grad=True)
    loss = _fused(lucid.orthogonal_loss_fn(t))
    (loss * k.sum()).backward()
    base = _run(inp["t"], dev)
    assert np.array_equal(_bits(t.grad.cpu().numpy()), _bits(base[1]))            # k.sum() = 1.5 exactly
    assert np.array_equal(_bits(k.grad.cpu().numpy()), _bits(np.repeat(base[0], 2)))
    _check("H with a tensor upstream", loss.detach().cpu().numpy().reshape(1), t.grad.cpu().numpy(), inp)


@pytest.mark.gpu
def test_views_and_two_dimensional_input(dev):
    """a transposed [h, d, n] leaf and a strided slice of a [2 n, d] leaf: the gradients arrive in the leaves' shapes"""
    from dynamicvectorquantization_amd import lucid
    inp = _inputs("H")
    base = _run(inp["t"], dev)
    leaf = _t(inp["t"].transpose(0, 2, 1), dev).requires_grad_(True)              # [h, d, n]
    view = leaf.transpose(1, 2)
    assert not view.is_contiguous()
    loss = _fused(lucid.orthogonal_loss_fn(view))
    (loss * UPSTREAM).backward()
    assert leaf.grad.shape == leaf.shape
    assert np.array_equal(_bits(loss.detach().cpu().numpy().reshape(1)), _bits(base[0]))
    assert np.array_equal(_bits(leaf.grad.transpose(1, 2).contiguous().cpu().numpy()), _bits(base[1]))
    # [n, d], every second row of a larger leaf
    one = _inputs("R")
    n, d = CASES["R"].n, CASES["R"].d
    big = np.zeros((2 * n, d), np.float32)
    big[::2] = one["t"][0]
    big[1::2] = 3.0
    leaf = _t(big, dev).requires_grad_(True)
    view = leaf[::2]
    assert view.shape == (n, d) and not view.is_contiguous()
    loss = _fused(lucid.orthogonal_loss_fn(view))
    (loss * UPSTREAM).backward()
    ref = _run(one["t"], dev)
    assert leaf.grad.shape == (2 * n, d) and not leaf.grad[1::2].any()
    assert np.array_equal(_bits(loss.detach().cpu().numpy().reshape(1)), _bits(ref[0]))
    assert np.array_equal(_bits(leaf.grad[::2].contiguous().cpu().numpy()), _bits(ref[1][0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("H", "L"))
def test_row_permutation(name, dev):
    c, inp = CASES[name], _inputs(name)
    head = c.h - 1
    perm = np.argsort(synth.uniform(c.seed + 50, (c.n,)), kind="stable")
    assert not np.array_equal(perm, np.arange(c.n)) and len(set(perm // 32 - np.arange(c.n) // 32)) > 1      # rows change tiles
    tp = inp["t"].copy()
    tp[head] = inp["t"][head][perm]
    g64p = inp["g64"].copy()
    g64p[head] = inp["g64"][head][perm]
    base, got = _run(inp["t"], dev), _run(tp, dev)
    _check("%s with the rows of head %d permuted" % (name, head), got[0], got[1], inp, g64p)
    assert abs(float(got[0][0]) - float(base[0][0])) <= 1e-6 * float(base[0][0])
    others = [i for i in range(c.h) if i != head]
    assert np.array_equal(_bits(got[1][others]), _bits(base[1][others]))
    # against the unpermuted run itself: both are within the bound of float64, so within twice the bound of each other
    scale = np.abs(UPSTREAM * inp["g64"]).max()
    assert np.abs(got[1][head].astype(np.float64) - base[1][head][perm]).max() <= 8.0 * inp["err32"] * scale
