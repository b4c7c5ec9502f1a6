"""GPU (-m gpu): fp16 / bf16 branch features through the routing tail (DVQ_FEATURES of include/dvq.h).
The contract is that of the 16-bit dense assign carried through the tail: every integer output is what the float32 op gives on
`x.float()`, codebook_mask and the gate logits stay float32, h_dual / h_triple come back in the input's dtype and hold exactly the
selected 16-bit values (a select moves bytes and rounds nothing).

(3) the selects, bit for bit against the oracle fed the widened arrays: h_out.float(), indices and codebook_mask are equal arrays,
    for the int64 gate, float32 logits (ties and NaN logits among them; at the shipped shape the golden's own) and the fixed-entropy
    router (whose int64 gate is returned as well), at shapes that reach every piece width: rows shorter than a piece and 8-byte
    planes, odd C, odd wc, wc % 4 == 0 (16-byte pieces over four coarse cells), the shipped shape, more than 4096 cells (no LDS
    grain map); and once with every feature tensor and out= buffer viewed one element into its storage.
(4) the feature-router gate: per row of tests/_gate_ref.CASES the module's no-grad forward on 16-bit branches under the project's
    rule (tests/_gate_ref.check_rule) against the float64 logits of the rounded values, the fp32 torch chain on the widened values as
    the yardstick; the float32 forward of the same module on the widened tensors gives the same bits (the pooling pass widens where
    it loads; everything behind the load is the float32 kernel), hence the same argmax on every clear cell.
(5) encode_dual / encode_triple end to end on 16-bit features equal the hand-composed chain (oracle select on the widened values ->
    the same conv call -> quantize(x=...)); without quant_conv and with the entropy router also the fused routed op on .float()
    features: same grain indices and codes, quant = that op's quant.to(dtype), emb_loss within 1e-5 relative."""
import copy
import os

import numpy as np
import pytest
import torch

from tests import _cases as C
from tests import _gate_ref as G
from tests import _route_x16_ref as X

pytestmark = pytest.mark.gpu

THR = 1.6777750253677368
SHAPES = [(1, 4, 1, 2), (2, 7, 1, 1),          # rows shorter than a piece, 8-byte planes
          (3, 5, 3, 6),                        # odd C
          (3, 6, 5, 7), (2, 32, 15, 15),       # odd wc
          (2, 8, 3, 4),                        # wc % 4 == 0: 16-byte pieces over four coarse cells
          (2, 256, 16, 16),                    # the shipped shape
          (1, 8, 65, 65)]                      # more than 4096 cells: no LDS grain map


def _spoil(logits, seed):
    """ties and NaN logits in a copy of float32 gate logits [B, hc, wc, G]: every 5th cell all equal, every 7th a NaN in one slot,
    every 11th NaN everywhere"""
    lg = logits.copy().reshape(-1, logits.shape[-1])
    n, g = lg.shape
    lg[0::5] = lg[0::5, :1]
    lg[np.arange(3, n, 7), (np.arange(3, n, 7) + seed) % g] = np.nan
    lg[6::11] = np.nan
    return lg.reshape(logits.shape)


def _wide(t):
    return t.float().cpu().numpy()


def _same(out, o, key, dtype, what):
    assert out[key].dtype == dtype and out["indices"].dtype == torch.int64 and out["codebook_mask"].dtype == torch.float32, what
    for k in (key, "indices", "codebook_mask"):
        got = _wide(out[k]) if k == key else out[k].cpu().numpy()
        assert got.shape == o[k].shape and np.array_equal(got, o[k], equal_nan=True), "%s: %s" % (what, k)


def _select_inputs(dev, dtype, shape):
    from dynamicvectorquantization_amd import synth
    B, Cc, hc, wc = shape
    t = lambda a: torch.from_numpy(a).to(dev)
    feats = {"c": t(synth.features(2, B, Cc, hc, wc)).to(dtype), "m": t(synth.features(5, B, Cc, 2 * hc, 2 * wc)).to(dtype),
             "f2": t(synth.features(1, B, Cc, 2 * hc, 2 * wc)).to(dtype), "f4": t(synth.features(4, B, Cc, 4 * hc, 4 * wc)).to(dtype)}
    gate = synth.grain_gate_dual(3, B, hc, wc)
    lg2 = _spoil(synth.normal(9, (B, hc, wc, 2)), 0)
    lg3 = _spoil(synth.grain_logits_triple(6, B, hc, wc), 1)
    gate3 = np.eye(3, dtype=np.int64)[np.argmax(synth.grain_logits_triple(6, B, hc, wc), -1)]
    ent = synth.entropy_map(7, B, hc, wc)
    ent.reshape(-1)[0::9] = np.float32(THR)
    ent.reshape(-1)[4::13] = np.nan
    return feats, gate, lg2, lg3, gate3, ent


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_select_bit_for_bit(dev, oracle_mod, shape, dtype):
    from dynamicvectorquantization_amd.router import route_select_dual, route_select_dual_entropy, route_select_triple
    B, Cc, hc, wc = shape
    t = lambda a: torch.from_numpy(a).to(dev)
    f, gate, lg2, lg3, gate3, ent = _select_inputs(dev, dtype, shape)
    duals = [("int64 gate", gate), ("float32 logits", lg2)]
    if shape == (2, 256, 16, 16):
        g = C.load("route_dual_B2")
        assert (int(g["B"]), int(g["C"])) == (B, Cc) and g["logits"].shape == (B, hc, wc, 2)
        duals.append(("the golden's logits", g["logits"]))
    for what, gt in duals:
        out = route_select_dual(t(gt), f["c"], f["f2"])
        _same(out, oracle_mod.route_select_dual(gt, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, " + what)
        assert tuple(out["gate"].shape) == (B, 2, hc, wc)
    og = oracle_mod.entropy_gate(ent, THR)
    out = route_select_dual_entropy(t(ent), THR, f["c"], f["f2"])
    _same(out, oracle_mod.route_select_dual(og, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, entropy router")
    assert out["gate"].dtype == torch.int64 and np.array_equal(out["gate"].cpu().numpy(), og.transpose(0, 3, 1, 2))
    for what, gt in (("float32 logits", lg3), ("int64 gate", gate3)):
        out = route_select_triple(t(gt), f["c"], f["m"], f["f4"])
        _same(out, oracle_mod.route_select_triple(gt, _wide(f["c"]), _wide(f["m"]), _wide(f["f4"])), "h_triple", dtype, "triple, " + what)
        assert tuple(out["gate"].shape) == (B, 3, hc, wc)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
def test_select_on_views_one_element_into_their_storage(dev, oracle_mod, dtype):
    """a tensor that starts one element into its storage is 2-byte aligned only (indices 8, codebook_mask 4): the same values, not
    a misaligned 16-byte access; the bytes around every out= buffer stay as they were"""
    from dynamicvectorquantization_amd.router import route_select_dual, route_select_dual_entropy, route_select_triple
    shape = (2, 8, 3, 4)                                       # rows and planes that would allow 16-byte pieces
    B, Cc, hc, wc = shape
    t = lambda a: torch.from_numpy(a).to(dev)
    f, gate, lg2, lg3, gate3, ent = _select_inputs(dev, dtype, shape)
    f = {k: X.offset_view(v) for k, v in f.items()}
    assert all(v.data_ptr() % 4 == 2 and v.is_contiguous() for v in f.values())

    def buffers(S, extra=()):
        """out= views one element into storages pre-filled with a sentinel, and the storages"""
        specs = [((B, Cc, S * hc, S * wc), dtype), ((B, hc, wc), torch.int64), ((B, 1, S * hc, S * wc), torch.float32)] + list(extra)
        stores = [torch.full((int(np.prod(s)) + 2,), 77, dtype=d, device=dev) for s, d in specs]
        return [st[1:-1].view(s) for st, (s, _) in zip(stores, specs)], stores

    def untouched(stores):
        return all(float(st[0]) == 77 and float(st[-1]) == 77 for st in stores)

    views, stores = buffers(2)
    out = route_select_dual(t(lg2), f["c"], f["f2"], out=tuple(views))
    assert out["h_dual"].data_ptr() == views[0].data_ptr() and views[0].data_ptr() % 4 == 2 and views[2].data_ptr() % 8 == 4
    _same(out, oracle_mod.route_select_dual(lg2, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, offset views")
    assert untouched(stores)
    views, stores = buffers(2, [((B, hc, wc, 2), torch.int64)])
    out = route_select_dual_entropy(t(ent), THR, f["c"], f["f2"], out=tuple(views))
    og = oracle_mod.entropy_gate(ent, THR)
    _same(out, oracle_mod.route_select_dual(og, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, entropy router, offset views")
    assert np.array_equal(views[3].cpu().numpy(), og) and untouched(stores)
    views, stores = buffers(4)
    out = route_select_triple(t(gate3), f["c"], f["m"], f["f4"], out=tuple(views))
    _same(out, oracle_mod.route_select_triple(gate3, _wide(f["c"]), _wide(f["m"]), _wide(f["f4"])), "h_triple", dtype, "triple, offset views")
    assert untouched(stores)
    with pytest.raises(TypeError, match="converts nothing"):
        route_select_dual(t(gate), f["c"], f["f2"], out=(views[0].float(), views[1], views[2]))


# ---- (4) the gate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("name", G.NAMES)
def test_gate_on_16_bit_branches(dev, name, dtype):
    inp = X.rounded(name, dtype)
    geo = inp.geo
    router, hs32 = G.on(inp, dev)
    hs16 = [h.to(dtype) for h in hs32]
    assert all(torch.equal(a.float(), b) for a, b in zip(hs16, hs32))
    got, t32 = G.run_kernel(inp, dev, router, hs16), G.run_torch32(inp, dev, router, hs32)
    assert tuple(got.shape) == (geo["B"], geo["hc"], geo["wc"], geo["nb"]) and got.dtype == torch.float32
    label = "%s %s" % (name, dtype)
    G.check_rule(got, t32, inp.logits64, slice_rule=name != G.ROW_OFFSET, label=label)
    f32 = G.run_kernel(inp, dev, router, hs32)
    ek, et, fl = G.image_errors(f32, t32, inp.logits64)
    clear = G.clear_cells(inp.logits64, et, fl).to(dev)
    assert torch.equal(got.argmax(-1)[clear], f32.argmax(-1)[clear]), label + ": another argmax than the float32 forward on a clear cell"
    assert torch.equal(got, f32), label + ": not the bits of the float32 op on the widened features"


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
def test_gate_rules_of_the_wrapper(dev, dtype):
    """branches of two dtypes raise; a branch that starts one element into its storage gives the same logits"""
    inp = X.rounded("r05", dtype)
    router, hs32 = G.on(inp, dev)
    hs16 = [h.to(dtype) for h in hs32]
    want = G.run_kernel(inp, dev, router, hs16)
    off = [X.offset_view(h) for h in hs16]
    assert all(h.data_ptr() % 8 != 0 for h in off)
    assert torch.equal(G.run_kernel(inp, dev, router, off), want)
    with pytest.raises(TypeError, match="one dtype"):
        G.run_kernel(inp, dev, router, [hs16[0], hs32[1]])
    with pytest.raises(TypeError, match="float32, float16 or bfloat16"):
        G.run_kernel(inp, dev, router, [h.double() for h in hs32])


# ---- (5) end to end --------------------------------------------------------------------------------------------------------------
def _vq(dev, K, D=64):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    E = synth.codebook_trained(K, D, seed=8801 + K)
    vq = VectorQuantize2(K, D).to(dev).eval()
    vq.codebook.weight.data[:-1].copy_(torch.from_numpy(E))
    return vq, E


def _conv(dev, dtype, D=64):
    from dynamicvectorquantization_amd import synth
    conv = torch.nn.Conv2d(D, D, 1).to(dev).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(synth.normal(8811, (D, D, 1, 1), 0.0, 1.0 / 8.0)))
        conv.bias.copy_(torch.from_numpy(synth.normal(8812, (D,), 0.0, 0.1)))
    return conv.to(dtype)


def _feature_router(dev, nb, C=64):
    from dynamicvectorquantization_amd.router import DualGrainFeatureRouter, TripleGrainFeatureRouter
    torch.manual_seed(8820 + nb)
    r = (DualGrainFeatureRouter if nb == 2 else TripleGrainFeatureRouter)(C, "group-8", "2layer-fc-SiLu").to(dev).eval()
    with torch.no_grad():
        for n_, p_ in r.named_parameters():
            if "feature_norm" in n_:
                p_.copy_(torch.randn_like(p_) * 0.5 + (1.0 if n_.endswith("weight") else 0.0))
    return r


def _check_chain(dev, dtype, got, osel, key, gate_want, conv, vq):
    """the outputs of encode_* against: oracle select (given) -> the same conv call -> quantize(x=...)"""
    quant, emb_loss, info, grain, gate = got
    h = torch.from_numpy(osel[key]).to(dev).to(dtype)
    assert np.array_equal(_wide(h), osel[key])                 # the selected 16-bit values, exactly
    with torch.no_grad():
        if conv is not None:
            h = conv(h)
        q, loss, (_, _, codes) = vq(x=h, codebook_mask=torch.from_numpy(osel["codebook_mask"]).to(dev))
    assert np.array_equal(grain.cpu().numpy(), osel["indices"]) and grain.dtype == torch.int64
    assert torch.equal(gate, gate_want)
    assert quant.dtype == dtype and torch.equal(quant, q) and torch.equal(info[2], codes)
    assert emb_loss.dtype == torch.float32 and torch.equal(emb_loss, loss)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("with_conv", [False, True], ids=["no-conv", "conv1x1"])
@pytest.mark.parametrize("K", [64, 1024])
def test_encode_dual_on_16_bit_features(dev, oracle_mod, golden_dir, K, with_conv, dtype):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.encode import encode_dual
    from dynamicvectorquantization_amd.router import DualGrainFixedEntropyRouter
    B, D, hc, wc = 3, 64, 5, 6
    vq, E = _vq(dev, K)
    conv = _conv(dev, dtype) if with_conv else None
    t = lambda a: torch.from_numpy(a).to(dev)
    hf, hcz = t(synth.z_tokens(E, B, 2 * hc, 2 * wc, 8831)).to(dtype), t(synth.z_tokens(E, B, hc, wc, 8832)).to(dtype)
    ent = synth.entropy_map(8833, B, hc, wc)
    fixed = DualGrainFixedEntropyRouter(os.path.join(golden_dir, "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
    with torch.no_grad():
        got = encode_dual(fixed, vq, hf, hcz, entropy=t(ent), quant_conv=conv)
    og = oracle_mod.entropy_gate(ent, fixed.fine_grain_threshold)
    osel = oracle_mod.route_select_dual(og, _wide(hcz), _wide(hf))
    assert len(np.unique(osel["indices"])) == 2
    _check_chain(dev, dtype, got, osel, "h_dual", t(og).permute(0, 3, 1, 2), conv, vq)
    if conv is None:
        # the float32 way: the fused routed op on the cast features (DESIGN.md section 4.19's contract between the two)
        with torch.no_grad():
            q32, loss32, info32, grain32, gate32 = encode_dual(fixed, vq, hf.float(), hcz.float(), entropy=t(ent))
        assert torch.equal(got[3], grain32) and torch.equal(got[2][2], info32[2]) and torch.equal(got[4], gate32)
        assert torch.equal(got[0], q32.to(dtype))
        assert abs(float(got[1]) - float(loss32)) <= 1e-5 * abs(float(loss32)), (float(got[1]), float(loss32))
    router = _feature_router(dev, 2)
    with torch.no_grad():
        got = encode_dual(router, vq, hf, hcz, quant_conv=conv)
        lg = router(h_fine=hf, h_coarse=hcz)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (B, hc, wc, 2)
    osel = oracle_mod.route_select_dual(lg.cpu().numpy(), _wide(hcz), _wide(hf))
    _check_chain(dev, dtype, got, osel, "h_dual", lg.permute(0, 3, 1, 2), conv, vq)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("with_conv", [False, True], ids=["no-conv", "conv1x1"])
@pytest.mark.parametrize("K", [64, 1024])
def test_encode_triple_on_16_bit_features(dev, oracle_mod, K, with_conv, dtype):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.encode import encode_triple
    B, D, hc, wc = 2, 64, 3, 5
    vq, E = _vq(dev, K)
    conv = _conv(dev, dtype) if with_conv else None
    t = lambda a: torch.from_numpy(a).to(dev)
    hf, hm, hcz = (t(synth.z_tokens(E, B, 4 * hc, 4 * wc, 8841)).to(dtype), t(synth.z_tokens(E, B, 2 * hc, 2 * wc, 8842)).to(dtype),
                   t(synth.z_tokens(E, B, hc, wc, 8843)).to(dtype))
    router = _feature_router(dev, 3)
    with torch.no_grad():
        got = encode_triple(router, vq, hf, hm, hcz, quant_conv=conv)
        lg = router(h_fine=hf, h_median=hm, h_coarse=hcz)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (B, hc, wc, 3)
    osel = oracle_mod.route_select_triple(lg.cpu().numpy(), _wide(hcz), _wide(hm), _wide(hf))
    _check_chain(dev, dtype, got, osel, "h_triple", lg.permute(0, 3, 1, 2), conv, vq)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
def test_what_still_raises(dev, golden_dir, dtype):
    """branches of two dtypes; 16-bit features that require grad through the select (named); the float32-only ops as before"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.encode import encode_dual, encode_triple
    from dynamicvectorquantization_amd.qconv import quant_conv_select
    from dynamicvectorquantization_amd.quantize import vq_assign_routed_dual
    from dynamicvectorquantization_amd.router import (DualGrainFixedEntropyRouter, route_select_dual, route_select_triple, route_train_dual)
    B, D, hc, wc = 2, 64, 3, 4
    vq, E = _vq(dev, 64)
    t = lambda a: torch.from_numpy(a).to(dev)
    hf, hm, hcz = (t(synth.features(8851, B, D, 4 * hc, 4 * wc)).to(dtype), t(synth.features(8852, B, D, 2 * hc, 2 * wc)).to(dtype),
                   t(synth.features(8853, B, D, hc, wc)).to(dtype))
    gate2, lg3 = t(synth.grain_gate_dual(8854, B, hc, wc)), t(synth.grain_logits_triple(8855, B, hc, wc))
    ent = t(synth.entropy_map(8856, B, hc, wc))
    fixed = DualGrainFixedEntropyRouter(os.path.join(golden_dir, "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
    other = torch.float16 if dtype == torch.bfloat16 else torch.bfloat16
    with torch.no_grad():
        for bad in (hcz.float(), hcz.to(other)):
            with pytest.raises(TypeError, match="one dtype"):
                route_select_dual(gate2, bad, hm)
            with pytest.raises(TypeError, match="one dtype"):
                route_select_triple(lg3, bad, hm, hf)
            with pytest.raises(TypeError, match="one dtype"):
                encode_dual(fixed, vq, hm, bad, entropy=ent)
            with pytest.raises(TypeError, match="one dtype"):
                encode_triple(lambda **kw: lg3, vq, hf, hm, bad)
        with pytest.raises(TypeError, match="must be float32"):
            vq_assign_routed_dual(hcz, hm, vq.codebook.codes, vq.codebook._prep, gate=gate2)
        with pytest.raises(TypeError, match="must be float32"):
            quant_conv_select(torch.nn.Conv2d(D, D, 1).to(dev), hcz, hm, gate=gate2)
    router = _feature_router(dev, 2)
    with pytest.raises(TypeError, match="must be float32"):
        route_train_dual(router, hm, hcz)
    with pytest.raises(TypeError, match="require grad must be float32"):
        route_select_dual(gate2, hcz.clone().requires_grad_(True), hm)
    with pytest.raises(TypeError, match="require grad must be float32"):
        route_select_triple(lg3, hcz, hm.clone().requires_grad_(True), hf)
    out = route_select_dual(gate2, hcz.float().requires_grad_(True), hm.float())      # float32 features: differentiable as before
    assert out["h_dual"].requires_grad
