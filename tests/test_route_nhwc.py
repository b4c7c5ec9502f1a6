"""GPU (-m gpu): channels_last branch features through the routing tail (DVQ_NHWC of include/dvq.h).

(1) the selects, dual and triple, float32 / fp16 / bf16, float32 logits (ties and NaN logits among them) and the int64 gate, bit
    for bit against the oracle's select on NCHW copies of the same values: h_out (channels_last, the input's dtype), indices and
    codebook_mask are equal arrays.  Shapes reach every piece width of route_select_rows_kernel (a pixel's run of 32 / 16 bytes: 16-byte
    pieces; 24: 8; 28 and 12: 4; 14: 2), a long run (C = 256), many cells of short runs (the kernel keeps no grain map, so there
    is one regime: 64 x 64 and 65 x 64 cells both run it), views one element into their storage, reused and refused out= buffers, a
    1 x 1 coarse branch (the same bytes in both layouts: not copied) and the fixed-entropy router.
(2) the feature-router gate on rows r01 - r13 and r17 of tests/_gate_ref.CASES (r14 / r15, the non-temporal form, once in float32):
    the module's no-grad forward on channels_last branches under the project's rule (tests/_gate_ref.check_rule) against the float64
    logits, the fp32 torch chain as the yardstick; fp16 / bf16 channels_last logits are the bits of the float32 channels_last op on
    the widened values; two runs give equal bits; a view that is misaligned for 16-byte pieces gives the same logits, and the
    narrower pieces the ABI serves for such a pointer stay under the rule.
(3) encode_dual (fixed-entropy and feature router) and encode_triple on fp16 / bf16 channels_last features, with and without a
    1 x 1 quant_conv, against the hand-composed chain on NCHW copies fed the same gate logits: codes, indices and gate equal, quant
    channels_last and equal, emb_loss within 1e-5 relative; float32 channels_last eval features give the codes and indices of their
    NCHW copies; autograd through route_select_dual on float32 channels_last features gives the NCHW gradients."""
import os

import numpy as np
import pytest
import torch

from tests import _gate_ref as G
from tests import _route_x16_ref as X

pytestmark = pytest.mark.gpu

CL = torch.channels_last
THR = 1.6777750253677368
DTYPES = [torch.float32] + X.DTYPES
IDS = ["fp32"] + X.IDS
#        B, C, hc, wc
SHAPES = [(2, 8, 3, 5),        # runs of 32 B (float32) / 16 B: 16-byte pieces
          (2, 6, 3, 5),        # 24 B: 8-byte pieces; 12 B: 4-byte
          (2, 7, 3, 5),        # 28 B: 4-byte pieces; 14 B: 2-byte
          (2, 256, 2, 2),      # a long run: 64 / 32 pieces per pixel
          (1, 2, 64, 64),      # 4096 cells, and one row of cells more: one regime (no grain map)
          (1, 2, 65, 64)]
GATE_ROWS = [n for n in G.NAMES if n not in ("r14", "r15", "r16")]


def _cl(t):
    return t.contiguous(memory_format=CL)


def _offset_cl(t):
    """t's values in a channels_last tensor that starts one element into a fresh storage"""
    B, C, H, W = t.shape
    buf = torch.full((t.numel() + 2,), 77, dtype=t.dtype, device=t.device)
    v = buf[1:-1].view(B, H, W, C).permute(0, 3, 1, 2)
    v.copy_(t)
    return v, buf


def _spoil(logits, seed):
    """ties and NaN logits in a copy of float32 gate logits [B, hc, wc, G]: every 5th cell all equal, every 7th a NaN in one slot (each
    slot in turn), every 11th NaN everywhere"""
    lg = logits.copy().reshape(-1, logits.shape[-1])
    n, g = lg.shape
    lg[0::5] = lg[0::5, :1]
    lg[np.arange(3, n, 7), (np.arange(3, n, 7) + seed) % g] = np.nan
    lg[6::11] = np.nan
    return lg.reshape(logits.shape)


def _wide(t):
    return t.float().cpu().numpy()


def _same(out, o, key, dtype, what, nhwc=True):
    assert out[key].dtype == dtype and out["indices"].dtype == torch.int64 and out["codebook_mask"].dtype == torch.float32, what
    if nhwc:
        assert out[key].is_contiguous(memory_format=CL), what + ": h_out is not channels_last"
    for k in (key, "indices", "codebook_mask"):
        got = _wide(out[k]) if k == key else out[k].cpu().numpy()
        assert got.shape == o[k].shape and np.array_equal(got, o[k], equal_nan=True), "%s: %s" % (what, k)


def _select_inputs(dev, dtype, shape):
    """NCHW feature tensors, gates and logits of one shape"""
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


# ---- (1) the selects ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("shape", SHAPES, ids=["x".join(map(str, s)) for s in SHAPES])
def test_select_bit_for_bit(dev, oracle_mod, shape, dtype):
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.router import _branch_features, route_select_dual, route_select_dual_entropy, route_select_triple
    B, Cc, hc, wc = shape
    t = lambda a: torch.from_numpy(a).to(dev)
    f, gate, lg2, lg3, gate3, ent = _select_inputs(dev, dtype, shape)
    c = {k: _cl(v) for k, v in f.items()}
    assert all(_lib.is_channels_last(v) for v in c.values())
    assert _branch_features([("h_coarse", c["c"]), ("h_fine", c["f2"])])[1] == _lib.FEATURES(dtype) | _lib.NHWC
    for what, gt in (("int64 gate", gate), ("float32 logits", lg2)):
        out = route_select_dual(t(gt), c["c"], c["f2"])
        _same(out, oracle_mod.route_select_dual(gt, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, " + what)
        assert tuple(out["gate"].shape) == (B, 2, hc, wc)
    og = oracle_mod.entropy_gate(ent, THR)
    out = route_select_dual_entropy(t(ent), THR, c["c"], c["f2"])
    _same(out, oracle_mod.route_select_dual(og, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, entropy router")
    assert out["gate"].dtype == torch.int64 and np.array_equal(out["gate"].cpu().numpy(), og.transpose(0, 3, 1, 2))
    nchw = route_select_dual_entropy(t(ent), THR, f["c"], f["f2"])                     # the same function on the NCHW copies
    assert torch.equal(out["h_dual"], nchw["h_dual"]) and torch.equal(out["indices"], nchw["indices"])
    assert torch.equal(out["codebook_mask"], nchw["codebook_mask"]) and torch.equal(out["gate"], nchw["gate"])
    for what, gt in (("float32 logits", lg3), ("int64 gate", gate3)):
        out = route_select_triple(t(gt), c["c"], c["m"], c["f4"])
        _same(out, oracle_mod.route_select_triple(gt, _wide(f["c"]), _wide(f["m"]), _wide(f["f4"])), "h_triple", dtype, "triple, " + what)
        assert tuple(out["gate"].shape) == (B, 3, hc, wc)
    # coarser branches that arrive NCHW are brought to the finest branch's layout
    out = route_select_triple(t(lg3), f["c"], f["m"], c["f4"])
    _same(out, oracle_mod.route_select_triple(lg3, _wide(f["c"]), _wide(f["m"]), _wide(f["f4"])), "h_triple", dtype, "triple, NCHW coarse / median")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_select_on_views_and_out_buffers(dev, oracle_mod, dtype):
    """every feature tensor and out= buffer one element into its storage: element-aligned only, so narrower pieces and the same
    values, and the bytes around every out= buffer stay as they were; out= buffers are reused; an NCHW out= raises"""
    from dynamicvectorquantization_amd.router import route_select_dual, route_select_dual_entropy, route_select_triple
    shape = (2, 8, 3, 5)                                       # runs that would allow 16-byte pieces
    B, Cc, hc, wc = shape
    es = torch.empty((), dtype=dtype).element_size()
    t = lambda a: torch.from_numpy(a).to(dev)
    f, gate, lg2, lg3, gate3, ent = _select_inputs(dev, dtype, shape)
    c = {k: _offset_cl(v)[0] for k, v in f.items()}
    assert all(v.data_ptr() % (2 * es) == es and v.is_contiguous(memory_format=CL) for v in c.values())

    def buffers(S, extra=()):
        h, store = _offset_cl(torch.zeros((B, Cc, S * hc, S * wc), dtype=dtype, device=dev))
        specs = [((B, hc, wc), torch.int64), ((B, 1, S * hc, S * wc), torch.float32)] + list(extra)
        stores = [torch.full((int(np.prod(s)) + 2,), 77, dtype=d, device=dev) for s, d in specs]
        return [h] + [st[1:-1].view(s) for st, (s, _) in zip(stores, specs)], [store] + stores

    def untouched(stores):
        return all(float(st[0]) == 77 and float(st[-1]) == 77 for st in stores)

    views, stores = buffers(2)
    for gt in (lg2, gate):                                     # the same buffers twice
        out = route_select_dual(t(gt), c["c"], c["f2"], out=tuple(views))
        assert out["h_dual"].data_ptr() == views[0].data_ptr()
        _same(out, oracle_mod.route_select_dual(gt, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, offset views")
        assert untouched(stores)
    views, stores = buffers(2, [((B, hc, wc, 2), torch.int64)])
    out = route_select_dual_entropy(t(ent), THR, c["c"], c["f2"], out=tuple(views))
    og = oracle_mod.entropy_gate(ent, THR)
    _same(out, oracle_mod.route_select_dual(og, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, entropy router, offset views")
    assert np.array_equal(views[3].cpu().numpy(), og) and untouched(stores)
    views, stores = buffers(4)
    out = route_select_triple(t(gate3), c["c"], c["m"], c["f4"], out=tuple(views))
    _same(out, oracle_mod.route_select_triple(gate3, _wide(f["c"]), _wide(f["m"]), _wide(f["f4"])), "h_triple", dtype, "triple, offset views")
    assert untouched(stores)
    nchw = torch.empty((B, Cc, 2 * hc, 2 * wc), dtype=dtype, device=dev)
    ind, cm = torch.empty((B, hc, wc), dtype=torch.int64, device=dev), torch.empty((B, 1, 2 * hc, 2 * wc), device=dev)
    with pytest.raises(ValueError, match="channels_last"):
        route_select_dual(t(gate), c["c"], c["f2"], out=(nchw, ind, cm))
    with pytest.raises(ValueError, match="channels_last"):
        route_select_dual_entropy(t(ent), THR, c["c"], c["f2"], out=(nchw, ind, cm, torch.empty((B, hc, wc, 2), dtype=torch.int64, device=dev)))
    with pytest.raises(ValueError, match="channels_last"):
        route_select_triple(t(gate3), c["c"], c["m"], c["f4"], out=(nchw, ind, cm))
    with pytest.raises(TypeError, match="converts nothing"):
        route_select_dual(t(gate), c["c"], c["f2"], out=(_cl(nchw).double(), ind, cm))


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_select_with_a_one_by_one_coarse_branch(dev, oracle_mod, dtype):
    """[B, C, 1, 1] is the same bytes in both layouts: served as it lies, whichever layout torch calls it"""
    from dynamicvectorquantization_amd.router import _branch_features, route_select_dual, route_select_triple
    shape = (3, 8, 1, 1)
    t = lambda a: torch.from_numpy(a).to(dev)
    f, gate, lg2, lg3, gate3, ent = _select_inputs(dev, dtype, shape)
    fine2, med, fine4 = _cl(f["f2"]), _cl(f["m"]), _cl(f["f4"])
    assert f["c"].is_contiguous() and f["c"].is_contiguous(memory_format=CL)
    hs, _ = _branch_features([("h_coarse", f["c"]), ("h_fine", fine2)])
    assert hs[0] is f["c"] and hs[1] is fine2
    out = route_select_dual(t(lg2), f["c"], fine2)
    _same(out, oracle_mod.route_select_dual(lg2, _wide(f["c"]), _wide(f["f2"])), "h_dual", dtype, "dual, 1 x 1 coarse")
    out = route_select_triple(t(lg3), f["c"], med, fine4)
    _same(out, oracle_mod.route_select_triple(lg3, _wide(f["c"]), _wide(f["m"]), _wide(f["f4"])), "h_triple", dtype, "triple, 1 x 1 coarse")


# ---- (2) the gate --------------------------------------------------------------------------------------------------------------
def _row(name, dtype):
    return G.case(name) if dtype == torch.float32 else X.rounded(name, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", GATE_ROWS)
def test_gate_on_channels_last_branches(dev, name, dtype):
    from dynamicvectorquantization_amd import _lib
    inp = _row(name, dtype)
    geo = inp.geo
    router, hs32 = G.on(inp, dev)
    hs = [_cl(h.to(dtype)) for h in hs32]
    assert _lib.is_channels_last(hs[-1]) and all(torch.equal(a.float(), b) for a, b in zip(hs, hs32))
    got, t32 = G.run_kernel(inp, dev, router, hs), G.run_torch32(inp, dev, router, hs32)
    assert tuple(got.shape) == (geo["B"], geo["hc"], geo["wc"], geo["nb"]) and got.dtype == torch.float32
    label = "%s %s channels_last" % (name, dtype)
    G.check_rule(got, t32, inp.logits64, label=label)
    assert torch.equal(G.run_kernel(inp, dev, router, hs), got), label + ": two runs differ"
    if dtype != torch.float32:
        f32 = G.run_kernel(inp, dev, router, [_cl(h) for h in hs32])
        assert torch.equal(got, f32), label + ": not the bits of the float32 channels_last op on the widened features"


@pytest.mark.parametrize("name", ["r14", "r15"])
def test_gate_non_temporal_form(dev, name):
    inp = G.case(name)
    router, hs32 = G.on(inp, dev)
    got, t32 = G.run_kernel(inp, dev, router, [_cl(h) for h in hs32]), G.run_torch32(inp, dev, router, hs32)
    G.check_rule(got, t32, inp.logits64, label=name + " float32 channels_last")


def _gate_abi(router, hs, flag):
    """dvq_router_gate_f32 called directly on a dual SiLU router behind GroupNorms (no wrapper: no copy of a misaligned view)"""
    from dynamicvectorquantization_amd import _lib
    B, C, hc, wc = hs[0].shape
    n = [router.feature_norm_coarse, router.feature_norm_fine]
    p = [t.detach().float().contiguous() for t in (n[0].weight, n[0].bias, n[1].weight, n[1].bias, router.gate[0].weight,
                                                  router.gate[0].bias, router.gate[2].weight, router.gate[2].bias)]
    hidden = p[4].shape[0]
    out = torch.empty((B, hc, wc, 2), dtype=torch.float32, device=hs[0].device)
    nbytes = _lib.checked.dvq_router_gate_workspace_bytes(2, B, C, hc, wc, n[0].num_groups, hidden)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=hs[0].device)
    _lib.checked.dvq_router_gate_f32(2, hs[0].data_ptr(), None, hs[1].data_ptr(), B, C, hc, wc, n[0].num_groups, float(n[0].eps),
                                     p[0].data_ptr(), p[1].data_ptr(), None, None, p[2].data_ptr(), p[3].data_ptr(), p[4].data_ptr(),
                                     p[5].data_ptr(), p[6].data_ptr(), p[7].data_ptr(), hidden, _lib.ACT_SILU | flag, None,
                                     out.data_ptr(), ws.data_ptr(), nbytes, _lib.stream_ptr(hs[0].device))
    return out


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("name", ["r05", "r10b"], ids=["r05-gemm-form", "r10b-direct-form"])
def test_gate_on_misaligned_views(dev, name, dtype):
    """through the module a view one element into its storage gives the aligned tensor's logits (the wrapper copies it); at the
    ABI the same view, and one two elements in, take narrower pieces (1 and 2 elements; 4 for a 16-bit view 8 bytes in) and stay
    under the rule"""
    from dynamicvectorquantization_amd import _lib
    inp = _row(name, dtype)
    router, hs32 = G.on(inp, dev)
    hs = [_cl(h.to(dtype)) for h in hs32]
    want, t32 = G.run_kernel(inp, dev, router, hs), G.run_torch32(inp, dev, router, hs32)
    off = [_offset_cl(h)[0] for h in hs]
    assert all(h.data_ptr() % 16 != 0 and _lib.is_channels_last(h) for h in off)
    assert torch.equal(G.run_kernel(inp, dev, router, off), want)
    flag = _lib.FEATURES(dtype) | _lib.NHWC
    G.check_rule(_gate_abi(router, hs, flag), t32, inp.logits64, label="%s %s, aligned, at the ABI" % (name, dtype))
    es = hs[0].element_size()
    for skip in sorted({1, 2, 8 // es}):                       # elements into the storage
        views = []
        for h in hs:
            B, C, H, W = h.shape
            buf = torch.empty(h.numel() + skip, dtype=h.dtype, device=dev)
            v = buf[skip:].view(B, H, W, C).permute(0, 3, 1, 2)
            v.copy_(h)
            views.append(v)
        G.check_rule(_gate_abi(router, views, flag), t32, inp.logits64, label="%s %s, %d elements in" % (name, dtype, skip))


# ---- (3) end to end ------------------------------------------------------------------------------------------------------------
B_, D_, HC, WC, K_ = 2, 64, 3, 4, 96


def _vq(dev):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import VectorQuantize2
    E = synth.codebook_trained(K_, D_, seed=8901)
    vq = VectorQuantize2(K_, D_).to(dev).eval()
    vq.codebook.weight.data[:-1].copy_(torch.from_numpy(E))
    return vq, E


def _conv(dev, dtype):
    from dynamicvectorquantization_amd import synth
    conv = torch.nn.Conv2d(D_, D_, 1).to(dev).eval()
    with torch.no_grad():
        conv.weight.copy_(torch.from_numpy(synth.normal(8911, (D_, D_, 1, 1), 0.0, 1.0 / 8.0)))
        conv.bias.copy_(torch.from_numpy(synth.normal(8912, (D_,), 0.0, 0.1)))
    return conv.to(dtype).to(memory_format=CL)


def _feature_router(dev, nb):
    from dynamicvectorquantization_amd.router import DualGrainFeatureRouter, TripleGrainFeatureRouter
    torch.manual_seed(8920 + nb)
    r = (DualGrainFeatureRouter if nb == 2 else TripleGrainFeatureRouter)(D_, "group-8", "2layer-fc-SiLu").to(dev).eval()
    with torch.no_grad():
        for n_, p_ in r.named_parameters():
            if "feature_norm" in n_:
                p_.copy_(torch.randn_like(p_) * 0.5 + (1.0 if n_.endswith("weight") else 0.0))
    return r


def _check_chain(got, sel, key, gate_want, conv, vq):
    """the outputs of encode_* on channels_last features against the chain composed by hand on NCHW copies: the NCHW select fed the
    SAME gate (given: its dict) -> the same conv call (torch's, on the layout encode_* hands it) -> quantize(x=...) on NCHW"""
    quant, emb_loss, info, grain, gate = got
    with torch.no_grad():
        h = sel[key]
        assert h.is_contiguous()
        if conv is not None:
            h = conv(_cl(h)).contiguous()
        q, loss, (_, _, codes) = vq(x=h, codebook_mask=sel["codebook_mask"])
    assert torch.equal(grain, sel["indices"]) and grain.dtype == torch.int64
    assert torch.equal(gate, gate_want)
    assert torch.equal(info[2], codes), "codes differ"
    assert quant.dtype == q.dtype and quant.is_contiguous(memory_format=CL) and not quant.is_contiguous(), "quant is not channels_last"
    assert torch.equal(quant.contiguous(), q.contiguous())
    assert emb_loss.dtype == torch.float32
    assert abs(float(emb_loss) - float(loss)) <= 1e-5 * abs(float(loss)), (float(emb_loss), float(loss))


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("with_conv", [False, True], ids=["no-conv", "conv1x1"])
def test_encode_dual_stays_channels_last(dev, golden_dir, with_conv, dtype):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.encode import encode_dual
    from dynamicvectorquantization_amd.router import DualGrainFixedEntropyRouter, entropy_gate, route_select_dual
    vq, E = _vq(dev)
    conv = _conv(dev, dtype) if with_conv else None
    t = lambda a: torch.from_numpy(a).to(dev)
    hf, hcz = t(synth.z_tokens(E, B_, 2 * HC, 2 * WC, 8931)).to(dtype), t(synth.z_tokens(E, B_, HC, WC, 8932)).to(dtype)
    ent = t(synth.entropy_map(8933, B_, HC, WC))
    fixed = DualGrainFixedEntropyRouter(os.path.join(golden_dir, "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
    with torch.no_grad():
        got = encode_dual(fixed, vq, _cl(hf), _cl(hcz), entropy=ent, quant_conv=conv)
        g64 = entropy_gate(ent, fixed.fine_grain_threshold)
        sel = route_select_dual(g64, hcz, hf)
    assert len(sel["indices"].unique()) == 2
    _check_chain(got, sel, "h_dual", g64.permute(0, 3, 1, 2), conv, vq)
    router = _feature_router(dev, 2)
    with torch.no_grad():
        got = encode_dual(router, vq, _cl(hf), _cl(hcz), quant_conv=conv)
        lg = got[4].permute(0, 2, 3, 1).contiguous()           # the logits the channels_last gate gave: the NCHW chain is fed the same
        sel = route_select_dual(lg, hcz, hf)
        assert torch.equal(router(h_fine=_cl(hf), h_coarse=_cl(hcz)), lg)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (B_, HC, WC, 2)
    _check_chain(got, sel, "h_dual", lg.permute(0, 3, 1, 2), conv, vq)


@pytest.mark.parametrize("dtype", X.DTYPES, ids=X.IDS)
@pytest.mark.parametrize("with_conv", [False, True], ids=["no-conv", "conv1x1"])
def test_encode_triple_stays_channels_last(dev, with_conv, dtype):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.encode import encode_triple
    from dynamicvectorquantization_amd.router import route_select_triple
    vq, E = _vq(dev)
    conv = _conv(dev, dtype) if with_conv else None
    t = lambda a: torch.from_numpy(a).to(dev)
    hf, hm, hcz = (t(synth.z_tokens(E, B_, 4 * HC, 4 * WC, 8941)).to(dtype), t(synth.z_tokens(E, B_, 2 * HC, 2 * WC, 8942)).to(dtype),
                   t(synth.z_tokens(E, B_, HC, WC, 8943)).to(dtype))
    router = _feature_router(dev, 3)
    with torch.no_grad():
        got = encode_triple(router, vq, _cl(hf), _cl(hm), _cl(hcz), quant_conv=conv)
        lg = got[4].permute(0, 2, 3, 1).contiguous()
        sel = route_select_triple(lg, hcz, hm, hf)
    assert lg.dtype == torch.float32 and tuple(lg.shape) == (B_, HC, WC, 3)
    _check_chain(got, sel, "h_triple", lg.permute(0, 3, 1, 2), conv, vq)


def test_float32_eval_features_keep_their_codes(dev, golden_dir):
    """float32 channels_last features in eval mode take the fused routed op as before (it copies inside): codes and indices of
    the NCHW copies"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.encode import encode_dual
    from dynamicvectorquantization_amd.router import DualGrainFixedEntropyRouter
    vq, E = _vq(dev)
    t = lambda a: torch.from_numpy(a).to(dev)
    hf, hcz = t(synth.z_tokens(E, B_, 2 * HC, 2 * WC, 8951)), t(synth.z_tokens(E, B_, HC, WC, 8952))
    ent = t(synth.entropy_map(8953, B_, HC, WC))
    fixed = DualGrainFixedEntropyRouter(os.path.join(golden_dir, "entropy_thresholds_imagenet_train_patch-16.json"), 0.5)
    with torch.no_grad():
        a = encode_dual(fixed, vq, _cl(hf), _cl(hcz), entropy=ent)
        b = encode_dual(fixed, vq, hf, hcz, entropy=ent)
    assert torch.equal(a[2][2], b[2][2]) and torch.equal(a[3], b[3]) and torch.equal(a[4], b[4])
    assert torch.equal(a[0].contiguous(), b[0].contiguous())


def test_autograd_through_the_select(dev):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.router import route_select_dual
    B, Cc, hc, wc = 2, 8, 3, 5
    t = lambda a: torch.from_numpy(a).to(dev)
    hcz, hf = t(synth.features(8961, B, Cc, hc, wc)), t(synth.features(8962, B, Cc, 2 * hc, 2 * wc))
    gate = t(synth.grain_gate_dual(8963, B, hc, wc))
    w = t(synth.normal(8964, (B, Cc, 2 * hc, 2 * wc)))
    grads = []
    for conv in (_cl, lambda x: x):
        a, b = conv(hcz).clone().requires_grad_(True), conv(hf).clone().requires_grad_(True)
        out = route_select_dual(gate, a, b)
        assert out["h_dual"].requires_grad
        (out["h_dual"] * w).sum().backward()
        grads.append((out["h_dual"].detach(), a.grad, b.grad))
    assert grads[0][0].is_contiguous(memory_format=CL) and not grads[0][0].is_contiguous()
    for x, y in zip(*grads):
        assert torch.equal(x.contiguous(), y.contiguous())
    assert float(grads[0][1].abs().sum()) > 0 and float(grads[0][2].abs().sum()) > 0
