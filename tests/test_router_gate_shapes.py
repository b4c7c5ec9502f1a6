"""GPU (-m gpu): the fused feature-router gate (csrc/router_gate.hip, fused_router_gate / dvq_router_gate_f32) at every form it
takes, against the float64 statement of the routers (tests/_gate_ref.py: the case table, the restated dispatch, the reference,
the rule; tests/test_router_gate_cases.py checks on the CPU that the table reaches the edges it names).

(a) per row, through the module under no_grad: shape [B, hc, wc, nb], every logit finite; per image
        err_kernel <= M * err_torch32 + 16 * 2^-24 * max |ref over the image|
    with both errors the largest absolute difference from float64 over the image, err_torch32 that of the module's own fp32
    torch-op forward on the same inputs on the same device (M: tests/_gate_ref.py, measured by tools/router_gate_accuracy.py into
    profiles/router_gate_accuracy.json); the argmax of float64 on every cell whose float64 top-2 margin exceeds
    2 * (M * err_torch32 + floor) of its image; and the old bar, 1e-4 * max(1, max |ref|), over the whole tensor.
    The offset row (group means 8 and 64 standard deviations from zero) is held to the old bar and the argmax condition only:
    the kernel folds the mean into an fp32 shift (bias - mean * rstd * w), which torch's (x - mean) * rstd does not, so its
    error grows with mean / spread where torch's does not (the gate's contract).  Measured on an MI355X
    (profiles/router_gate_accuracy.json, row r16): err_kernel 1.63e-6 against err_torch32 9.0e-7 at max |ref| 0.41, 6.7 times
    the floor; the slice rule would have needed m = 2.64 there.
(b) dvq_router_gate_f32 called directly -- without prepared weight images, with dvq_router_gate_prepare_f32 only, with
    dvq_router_gate_prepare_norm_f32 as well: every output element written and finite (output pre-filled with NaN, workspace and
    prep with NaN bytes), nothing around them touched (64 sentinel floats on either side of the output, 4096 sentinel bytes
    behind the workspace), rule (a) on each, and a second call on the same workspace bitwise equal to the first.  In the GEMM
    form the feature images of a partial last cell block are finite in their unused cell columns too.
(c) the module's cache of the weight images: after an in-place update of gate[0].weight and of a GroupNorm weight in eval mode
    the next call follows the new parameters (rule (a) against them); two calls without a change are bitwise equal.
(d) a NaN in one feature of one image leaves every other image's logits bitwise as they were and, without normalisation, every
    other cell of that image too."""
import pytest
import torch

from dynamicvectorquantization_amd import _lib
from tests import _gate_ref as G

pytestmark = pytest.mark.gpu


def _ncu(dev):
    return torch.cuda.get_device_properties(dev).multi_processor_count


@pytest.mark.parametrize("name", G.NAMES)
def test_logits_vs_float64(dev, name):
    inp = G.case(name)
    geo = G.dispatch(inp.case, _ncu(dev))
    if _ncu(dev) == 256:
        assert geo == inp.geo
    router, hs = G.on(inp, dev)
    got, t32 = G.run_kernel(inp, dev, router, hs), G.run_torch32(inp, dev, router, hs)
    assert tuple(got.shape) == (geo["B"], geo["hc"], geo["wc"], geo["nb"]) and got.dtype == torch.float32
    G.check_rule(got, t32, inp.logits64, slice_rule=name != G.ROW_OFFSET, label=name)


# ---- (b) the ABI entry point, guarded ------------------------------------------------------------------------------------------
GUARD, WS_GUARD = 64, 4096
SENT_F, SENT_B = 12345.0, 0xA5


def _abi_tensors(router, nb):
    """GroupNorm weight / bias coarse, median, fine, then w1, b1, w2, b2 in the ABI's order (None where the router has none)"""
    out = []
    for n in ("coarse", "median", "fine"):
        norm = getattr(router, "feature_norm_" + n, None) if (nb == 3 or n != "median") else None
        gn = isinstance(norm, torch.nn.GroupNorm)
        out += [norm.weight if gn else None, norm.bias if gn else None]
    g = router.gate
    out += [None, None, g.weight, g.bias] if isinstance(g, torch.nn.Linear) else [g[0].weight, g[0].bias, g[2].weight, g[2].bias]
    return [None if p is None else p.detach().contiguous() for p in out]


@pytest.mark.parametrize("name", G.ABI_ROWS)
def test_abi_call_writes_every_logit_and_nothing_else(dev, name):
    inp = G.case(name)
    d = G.dispatch(inp.case, _ncu(dev))
    nb, B, C, hc, wc, groups = d["nb"], d["B"], d["C"], d["hc"], d["wc"], d["groups"]
    assert d["act"] != 0
    router, hs = G.on(inp, dev)
    t32 = G.run_torch32(inp, dev, router, hs)
    params = _abi_tensors(router, nb)
    ptr, checked, stream = _lib.ptr, _lib.checked, _lib.stream_ptr(dev)
    ws_bytes = checked.dvq_router_gate_workspace_bytes(*G.abi_size_args(d))
    prep_bytes = checked.dvq_router_gate_prep_bytes(nb, C, d["Hid"])
    assert (ws_bytes, prep_bytes) == (d["ws_bytes"], d["prep_bytes"])
    n = B * hc * wc * nb
    out = torch.full((n + 2 * GUARD,), SENT_F, dtype=torch.float32, device=dev)
    view = out[GUARD:GUARD + n]
    ways = ["in-call images", "prepared images"] + (["prepared images and GroupNorm maxima"] if groups > 0 else [])
    for way in ways:
        ws = torch.full((ws_bytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=dev)      # NaN bytes: a read of unwritten scratch shows
        ws[ws_bytes:] = SENT_B
        prep = None
        if way != "in-call images":
            prep = torch.full((prep_bytes + WS_GUARD,), 0xFF, dtype=torch.uint8, device=dev)
            prep[prep_bytes:] = SENT_B
            assert prep.data_ptr() % 256 == 0
            checked.dvq_router_gate_prepare_f32(ptr(params[6]), nb, C, d["Hid"], prep.data_ptr(), prep_bytes, stream)
            if way.endswith("maxima"):
                checked.dvq_router_gate_prepare_norm_f32(nb, C, d["Hid"], *[ptr(p) for p in params[:6]], prep.data_ptr(), prep_bytes,
                                                         stream)
        assert ws.data_ptr() % 256 == 0
        runs = []
        for _ in range(2):
            view.fill_(float("nan"))
            checked.dvq_router_gate_f32(nb, ptr(hs[0]), ptr(hs[1]) if nb == 3 else None, ptr(hs[-1]), B, C, hc, wc, groups, 1e-6,
                                        *[ptr(p) for p in params], d["Hid"], d["act"], ptr(prep), view.data_ptr(), ws.data_ptr(),
                                        ws_bytes, stream)
            torch.cuda.synchronize()
            assert bool((out[:GUARD] == SENT_F).all()), way + ": written before the output"
            assert bool((out[GUARD + n:] == SENT_F).all()), way + ": written behind the output"
            left = int(torch.isnan(view).sum())
            assert left == 0, "%s: %d of %d logits never written (or NaN)" % (way, left, n)
            assert bool((ws[ws_bytes:] == SENT_B).all()), way + ": written behind the workspace"
            assert prep is None or bool((prep[prep_bytes:] == SENT_B).all()), way + ": written behind the prep buffer"
            runs.append(view.clone().reshape(B, hc, wc, nb))
        if d["gemm_form"] and d["memset"]:
            # the feature images of the last, partial cell block: its unused cell columns ride through the matrix cores with the
            # live ones and must hold finite values, whatever the workspace held before
            off = G.a256(B * d["F"] * 8) + (d["nblocks"] - 1) * d["S16"] * 2048
            last = ws[off:off + d["S16"] * 2048].view(torch.float16)
            assert bool(torch.isfinite(last).all()), way + ": non-finite operand columns in the last cell block's feature images"
        assert torch.equal(runs[0], runs[1]), way + ": the second call on the same workspace differs"
        G.check_rule(runs[0], t32, inp.logits64, label="%s, %s" % (name, way))


# ---- (c) the module's cache of the weight images -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["r06", "r03"], ids=["gemm-form", "direct-form"])
def test_module_cache_follows_in_place_parameter_updates(dev, name):
    inp = G.case(name)
    router, hs = G.on(inp, dev)
    assert not router.training
    first = G.run_kernel(inp, dev, router, hs)
    assert torch.equal(first, G.run_kernel(inp, dev, router, hs)), "two calls without a change differ"
    G.check_rule(first, G.run_torch32(inp, dev, router, hs), inp.logits64, label=name)
    g = torch.Generator(device="cpu").manual_seed(5)
    with torch.no_grad():
        for p in (router.gate[0].weight, router.feature_norm_fine.weight):
            p.mul_((1.0 + 0.5 * torch.randn(p.shape, generator=g)).to(dev))          # in place: same storage, a new version
            ref = G.reference64(inp, router)
            assert float((ref - inp.logits64).abs().max()) > 1e-3, "the update does nothing"
            got = G.run_kernel(inp, dev, router, hs)
            G.check_rule(got, G.run_torch32(inp, dev, router, hs), ref, label=name + ", updated")
            assert torch.equal(got, G.run_kernel(inp, dev, router, hs))


# ---- (d) non-finite isolation --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm", ["row", "none"])
@pytest.mark.parametrize("name", G.NAN_ROWS)
def test_a_nan_stays_in_its_image(dev, name, norm):
    c = G.row(name)
    if norm == "none":
        c = c[:6] + ("none",) + c[7:]
        assert not G.dispatch(c)["gemm_form"]
    inp = G.case(name) if norm == "row" else G.Inputs(c)
    geo = inp.geo
    router, hs = G.on(inp, dev)
    clean = G.run_kernel(inp, dev, router, hs)
    assert bool(torch.isfinite(clean).all())
    b, y, x = geo["B"] - 1, geo["hc"] - 1, 1                 # a cell of the last image, in the finest branch
    s = 1 << (geo["nb"] - 1)
    hs[-1][b, geo["C"] // 2, s * y + 1, s * x] = float("nan")
    got = G.run_kernel(inp, dev, router, hs)
    assert torch.equal(got[:b], clean[:b]), "a NaN in image %d changed another image's logits" % b
    assert bool(torch.isnan(got[b, y, x]).all()), "the NaN did not reach its own cell"
    if norm == "none":
        keep = torch.ones((geo["hc"], geo["wc"]), dtype=torch.bool, device=dev)
        keep[y, x] = False
        assert torch.equal(got[b][keep], clean[b][keep]), "without normalisation a NaN changed another cell of its image"


# ---- what the direct form's LDS cannot hold ------------------------------------------------------------------------------------
def test_oversize_router_is_refused_in_words_before_anything_is_allocated(dev):
    """a default triple router of C = 384 needs 165888 bytes for its feature tile and output-layer rows: the module raises with the
    condition in its message (the ABI's own words: tests/golden/abi_rejections.json); C = 376, the widest that fits, is served
    under rule (a)"""
    wide = ("c376", 3, 2, 376, 4, 4, "none", G.SILU, None, 376, None, "the widest default triple router the direct form holds")
    d = G.dispatch(wide)
    assert not d["gemm_form"] and d["lds"] <= G.GATE_LDS_MAX < G.direct_lds_bytes(3, 384, 4, 4, 0, 3 * 384, 1)
    inp = G.Inputs(wide)
    router, hs = G.on(inp, dev)
    G.check_rule(G.run_kernel(inp, dev, router, hs), G.run_torch32(inp, dev, router, hs), inp.logits64, label="c376")
    inp = G.Inputs(wide[:3] + (384,) + wide[4:])
    router, hs = G.on(inp, dev)
    free = torch.cuda.memory_allocated(dev)
    with pytest.raises(_lib.DvqError, match="fit the LDS"):
        G.run_kernel(inp, dev, router, hs)
    assert torch.cuda.memory_allocated(dev) == free
