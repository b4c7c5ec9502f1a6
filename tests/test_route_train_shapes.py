"""GPU (-m gpu): the training-mode routing tail (csrc/router_train.hip, route_train_dual / route_train_triple) at ragged shapes,
against the float64 statement of the op (tests/_route_train_ref.py: the case table, the reference, the slice rule;
tests/test_route_train_cases.py checks on the CPU that the table reaches the edges it names and that its decisions are clear).

(a) per row: indices, codebook_mask and the gate's zero pattern identical to float64's; the gate on the hard index within 2 fp32
    ulp of the float64 value rounded to fp32; h_out 1e-6 relative; every gradient, per slice (each (image, channel) plane of each
    dh, each row of dW1 / dW2, the whole vector for biases and GroupNorm gradients):
        err_kernel <= m * err_torch32 + 16 * 2^-24 * max |ref over the slice|
    with both errors the largest absolute difference from float64 over the slice, err_torch32 that of the package's own fp32
    torch-op chain on the same inputs on the same device.  m = 3 (M), the factor test_feature_router_logits_large_groupnorm_parameters
    uses for the same kind of comparison, for every tensor (measured: profiles/route_train_accuracy.json,
    tools/route_train_accuracy.py).  No tensor is further than 1e-4 * max |ref| (the bar
    of tests/test_route_train.py) either.
(b) the two ABI entry points called directly: every output element is written (outputs pre-filled with NaN / -1, the workspace
    with NaN bytes), and nothing around them is (64 sentinel elements on either side of every output, 4096 sentinel bytes behind
    the workspace); twice on one workspace.
(c) tau in {0.5, 2.0}: the decisions of tau = 1 under the same noise, the gradients under rule (a).
(d) saved state: backward twice, two forwards with their backwards in the opposite order, the slab sums run to run: bitwise."""
import pytest
import torch
import torch.nn as nn

from dynamicvectorquantization_amd import _lib
from tests import _route_train_ref as R

pytestmark = pytest.mark.gpu

ROWS = list(range(len(R.CASES))) + [-1]
IDS = [R.case_id(r) for r in R.CASES] + ["no-update"]
M = 3.0
# No tensor gets another m for its fixed-order serial fp32 sum: measured on an MI355X (profiles/route_train_accuracy.json) the
# largest m any slice of any row needs is 1.76 (dW1, the 105-cell row), then 1.31 (dh_coarse, pseudo-groups) and 0.015 (dgamma of
# the median branch); every other tensor, the candidates rt_cellsum_kernel (sums over cells), rt_coef_kernel (over images) and
# rt_dgg_kernel (over channels) included, stays inside the sixteen-rounding floor on every slice.


def _check(inp, ref, ker, t32):
    cpu = lambda t: t.detach().cpu()
    assert torch.equal(cpu(t32["indices"]), ref["indices"]), "condition: the fp32 torch chain takes float64's decisions"
    assert torch.equal(cpu(ker["indices"]), ref["indices"]), "indices"
    assert torch.equal(cpu(ker["codebook_mask"]), ref["codebook_mask"]), "codebook_mask"
    assert tuple(ker["gate"].shape) == tuple(ref["gate"].shape)
    if inp.update_router:
        R.check_gate(cpu(ker["gate"]), ref["gate"].float(), True)
    R.check_h(cpu(ker["h"]).double(), ref["h"])
    items = list(ref["grads"].items()) + ([] if inp.update_router else [("gate", ref["gate"])])
    worst, bad = (0.0, ""), []
    for name, r in items:
        got = ker["gate"] if name == "gate" else ker["grads"][name]
        t = t32["gate"] if name == "gate" else t32["grads"][name]
        assert tuple(got.shape) == tuple(r.shape), name
        ek, et, fl = R.slice_errors(got, t, r)
        need = R.m_needed(ek, et, fl)
        print("%-28s err_kernel %.3g err_torch32 %.3g max|ref| %.3g m needed %.3g"
              % (name, float(ek.max()), float(et.max()), float(r.abs().max()), need))
        worst = max(worst, (need, name))
        fail = (ek > M * et + fl).nonzero().flatten().tolist()
        if fail:
            j = fail[0]
            bad.append("%s: %d slices, first %d: err_kernel %.3g > %g * %.3g + %.3g" % (name, len(fail), j, float(ek[j]), M,
                                                                                       float(et[j]), float(fl[j])))
        if float(ek.max()) > 1e-4 * float(r.abs().max()):
            bad.append("%s: %.3g beyond 1e-4 * max |ref| = %.3g" % (name, float(ek.max()), 1e-4 * float(r.abs().max())))
    print("worst m needed: %.3g (%s)" % worst)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("i", ROWS, ids=IDS)
def test_forward_backward_vs_float64(dev, i):
    inp, ref = R.case(i)
    _check(inp, ref, R.run_kernel(inp, dev), R.run_torch32(inp, dev))


@pytest.mark.parametrize("tau", [0.5, 2.0])
@pytest.mark.parametrize("i", [R.ROW_105, R.ROW_F24], ids=["dual", "triple"])
def test_tau(dev, i, tau):
    """softmax is monotone: the decisions of tau = 1 under the same noise; a dropped or doubled 1 / tau shows in the gradients"""
    inp, ref = R.case(i, tau)
    one, ref1 = R.case(i, 1.0)
    assert inp.tau == tau and one.tau == 1.0 and torch.equal(inp.gumbels, one.gumbels)
    assert torch.equal(ref["indices"], ref1["indices"])
    w2 = "gate.2.weight"
    assert float((ref["grads"][w2] - ref1["grads"][w2]).abs().max()) > 0.1 * float(ref1["grads"][w2].abs().max()), "tau does nothing"
    ker = R.run_kernel(inp, dev)
    assert torch.equal(ker["indices"].cpu(), R.run_kernel(one, dev)["indices"].cpu())
    _check(inp, ref, ker, R.run_torch32(inp, dev))


# ---- (b) the ABI entry points, guarded ----------------------------------------------------------------------------------------
GUARD, WS_GUARD = 64, 4096
SENT_F, SENT_I, SENT_B = 12345.0, -7, 0xA5


class _Guarded:
    """an output of n elements inside a buffer with GUARD sentinel elements on either side, pre-filled with NaN / -1"""

    def __init__(self, shape, dtype, dev):
        self.n = 1
        for s in shape:
            self.n *= s
        self.shape, self.fp = shape, dtype.is_floating_point
        self.buf = torch.full((self.n + 2 * GUARD,), SENT_F if self.fp else SENT_I, dtype=dtype, device=dev)
        self.view = self.buf[GUARD:GUARD + self.n]
        self.refill()

    def refill(self):
        self.view.fill_(float("nan") if self.fp else -1)

    def ptr(self):
        return self.view.data_ptr()

    def check(self, name):
        sent = SENT_F if self.fp else SENT_I
        assert bool((self.buf[:GUARD] == sent).all()), name + ": written before the output"
        assert bool((self.buf[GUARD + self.n:] == sent).all()), name + ": written behind the output"
        left = int(torch.isnan(self.view).sum()) if self.fp else int((self.view == -1).sum())
        assert left == 0, "%s: %d of %d elements never written" % (name, left, self.n)
        return self.view.clone().reshape(self.shape)


def _params(router, nb):
    """the router's parameters in the ABI's order: GroupNorm weight / bias coarse, median, fine; w1, b1, w2, b2"""
    out = []
    for n in ("coarse", "median", "fine"):
        norm = getattr(router, "feature_norm_" + n, None) if (nb == 3 or n != "median") else None
        gn = isinstance(norm, nn.GroupNorm)
        out += [("feature_norm_%s.weight" % n, norm.weight if gn else None), ("feature_norm_%s.bias" % n, norm.bias if gn else None)]
    g = router.gate
    if isinstance(g, nn.Linear):
        out += [(None, None), (None, None), ("gate.weight", g.weight), ("gate.bias", g.bias)]
    else:
        out += [("gate.0.weight", g[0].weight), ("gate.0.bias", g[0].bias), ("gate.2.weight", g[2].weight), ("gate.2.bias", g[2].bias)]
    return [(n, None if p is None else p.detach().contiguous()) for n, p in out]


@pytest.mark.parametrize("i", [R.ROW_105, R.ROW_WO258, R.ROW_N513], ids=["105-cells", "Wo258", "513-cells"])
def test_every_output_element_is_written_and_nothing_else(dev, i):
    inp, _ = R.case(i)
    g = inp.geo
    nb, B, C, hc, wc, S = g["nb"], g["B"], g["C"], g["hc"], g["wc"], g["S"]
    router, hs, gum, Rc, Qc = R._on(inp, dev)
    want = R.run_kernel(inp, dev)                                        # the same call through autograd
    hs3 = [hs[0].detach(), hs[1].detach() if nb == 3 else None, hs[-1].detach()]
    params = _params(router, nb)
    ptr = _lib.ptr
    args = ([nb] + [ptr(t) for t in hs3] + [B, C, hc, wc, g["groups"], 1e-6] + [ptr(p) for _, p in params]
            + [g["H"], g["act"], ptr(gum), inp.tau])
    ws_bytes = _lib.checked.dvq_route_train_workspace_bytes(nb, B, C, hc, wc, g["groups"], g["H"])
    assert ws_bytes == R.rt_layout_total(nb, B, C, hc, wc, g["groups"], g["H"])
    ws = torch.full((ws_bytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=dev)     # NaN bytes: a read of unwritten scratch shows
    ws[ws_bytes:] = SENT_B
    assert ws.data_ptr() % 256 == 0
    f32, i64 = torch.float32, torch.int64
    fwd = {"h": _Guarded((B, C, S * hc, S * wc), f32, dev), "indices": _Guarded((B, hc, wc), i64, dev),
           "codebook_mask": _Guarded((B, 1, S * hc, S * wc), f32, dev), "gate": _Guarded((B, hc, wc, nb), f32, dev)}
    dh = [None if h is None else _Guarded(tuple(h.shape), f32, dev) for h in hs3]
    dp = [None if p is None else _Guarded(tuple(p.shape), f32, dev) for _, p in params]
    g_out, g_gate = Rc.contiguous(), Qc.permute(0, 2, 3, 1).contiguous()               # d gate in the kernel's [B, hc, wc, nb]
    stream = _lib.stream_ptr(dev)
    runs = []
    for _ in range(2):
        for o in list(fwd.values()) + [o for o in dh + dp if o is not None]:
            o.refill()
        _lib.checked.dvq_route_train_forward_f32(*args, fwd["h"].ptr(), fwd["indices"].ptr(), fwd["codebook_mask"].ptr(),
                                                 fwd["gate"].ptr(), ws.data_ptr(), ws_bytes, stream)
        _lib.checked.dvq_route_train_backward_f32(*args, g_out.data_ptr(), g_gate.data_ptr(), ws.data_ptr(), ws_bytes,
                                                  *[0 if o is None else o.ptr() for o in dh],
                                                  *[0 if o is None else o.ptr() for o in dp], stream)
        torch.cuda.synchronize()
        got = {k: o.check(k) for k, o in fwd.items()}
        for name, o in zip(["h_coarse", "h_median", "h_fine"], dh):
            if o is not None:
                got[name] = o.check("d" + name)
        for (name, _), o in zip(params, dp):
            if o is not None:
                got[name] = o.check("d " + name)
        assert bool((ws[ws_bytes:] == SENT_B).all()), "written behind the workspace"
        runs.append(got)
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k + ": the second call on the same workspace differs"
    got = runs[0]
    for k in ("h", "indices", "codebook_mask"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["gate"].permute(0, 3, 1, 2), want["gate"])
    assert set(want["grads"]) == set(got) - set(fwd)
    for k, v in want["grads"].items():
        assert torch.equal(got[k], v), k


# ---- (d) saved state ----------------------------------------------------------------------------------------------------------
def _forward(inp, dev):
    _, loss, leaves = R.kernel_graph(inp, dev)
    return loss, leaves


def _same(a, b, what):
    assert len(a) == len(b)
    for j, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), "%s: gradient %d differs" % (what, j)


def test_backward_twice_is_bit_identical(dev):
    inp, _ = R.case(R.ROW_N513)
    loss, leaves = _forward(inp, dev)
    g1 = [g.clone() for g in torch.autograd.grad(loss, leaves, retain_graph=True)]
    g2 = torch.autograd.grad(loss, leaves, retain_graph=True)
    _same(g1, g2, "second backward")
    _same(g1, [R.run_kernel(inp, dev)["grads"][n] for n in inp.names()], "a fresh forward + backward")


def test_two_forwards_backwards_in_the_opposite_order(dev):
    """each forward's saved state is its own: two rows of different shapes, backward in the opposite order, against each alone"""
    a, _ = R.case(R.ROW_105)
    b, _ = R.case(3)
    la, leaves_a = _forward(a, dev)
    lb, leaves_b = _forward(b, dev)
    gb = torch.autograd.grad(lb, leaves_b)
    ga = torch.autograd.grad(la, leaves_a)
    _same(ga, [R.run_kernel(a, dev)["grads"][n] for n in a.names()], "first forward, second backward")
    _same(gb, [R.run_kernel(b, dev)["grads"][n] for n in b.names()], "second forward, first backward")
    # and the same shape with other inputs: the workspace of the first is not the second's
    c = R.Inputs(R.CASES[R.ROW_105], 77)
    la, leaves_a = _forward(a, dev)
    lc, leaves_c = _forward(c, dev)
    gc = torch.autograd.grad(lc, leaves_c)
    ga2 = torch.autograd.grad(la, leaves_a)
    _same(ga2, ga, "same shape, other inputs in between")
    _same(gc, [R.run_kernel(c, dev)["grads"][n] for n in c.names()], "same shape, other inputs")


@pytest.mark.parametrize("i", [R.ROW_N513, R.ROW_N8320], ids=["513-cells", "8320-cells"])
def test_slab_sums_are_bitwise_deterministic(dev, i):
    inp, _ = R.case(i)
    r1, r2 = R.run_kernel(inp, dev), R.run_kernel(inp, dev)
    for k in ("h", "indices", "codebook_mask", "gate"):
        assert torch.equal(r1[k], r2[k]), k
    for k in r1["grads"]:
        assert torch.equal(r1["grads"][k], r2["grads"][k]), k
