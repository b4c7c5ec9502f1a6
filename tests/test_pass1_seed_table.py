"""GPU (-m gpu): pass 1's accumulator seeds come from a table resident in LDS when a workgroup's code tiles fit it (K <= 1024, or a
slice that small of the split form) and travel with every tile otherwise (csrc/dvq_pass1.h, pass1_body RES).  The seeds
are the same fp32 values read from another address, so every form of pass 1 must still give the oracle's bits on both sides of
the limit: K = 32 (one tile), K not a multiple of 32, K = 1024 (the table exactly fills the seeds area), K = 1056 / 2048 below
131 072 tokens (the per-tile form must be taken and be right).  Ops: routed dual / triple (staged select), dense (cached / plain),
CONV, FOLD, row-major (flat) and the split form (<= 8192 tokens).  Bar: codes, grain indices, codebook_mask and z_q bit-exact, loss
1e-5 (tests/_cases.loss_close); the resolver queue's counts on the bench step's inputs equal the parent commit's."""
import numpy as np
import pytest
import torch

from tests import _cases as C

pytestmark = pytest.mark.gpu

THR = 1.6777750253677368
KS = [32, 333, 1024, 1056, 2048]
# (queued, listed) of prep.fallback_count() after the bench step (routed dual op, B = 256, K = 1024, slot 0's inputs), taken from a
# run of the parent commit's library on the same inputs: counts, not tolerances
PARENT_BENCH_FALLBACK = (5853, 0)


def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _check_routed(r, o_sel, o, B, oracle_mod):
    assert np.array_equal(r["indices"].cpu().numpy(), o_sel["indices"]), "grain indices"
    assert np.array_equal(r["codebook_mask"].cpu().numpy(), o_sel["codebook_mask"]), "codebook_mask"
    assert np.array_equal(r["codes"].cpu().numpy().reshape(B, -1), o["codes"]), "codes"
    assert np.array_equal(r["zq"].cpu().numpy(), o["zq"], equal_nan=True), "z_q"
    assert C.loss_close(float(r["loss"][1]), oracle_mod.vq_loss(o["sqerr"], o["numel"], 0.25)), "loss"


@pytest.mark.parametrize("B", [2, 12])                       # 2048 positions: split form (per-lane select); 12288: staged select
@pytest.mark.parametrize("K", KS)
def test_routed_dual(dev, oracle_mod, K, B):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_dual
    D = 256
    E = synth.codebook_trained(K, D, seed=1200 + K)
    hf, hc = synth.z_tokens(E, B, 32, 32, 1210 + K), synth.z_tokens(E, B, 16, 16, 1220 + K)
    ent = synth.entropy_map(1230 + K, B, 16, 16)
    t = _t(dev)
    prep = _CodebookPrep()
    r = vq_assign_routed_dual(t(hc), t(hf), t(E), prep, entropy=t(ent), threshold=THR)
    og = oracle_mod.entropy_gate(ent, THR)
    o_sel = oracle_mod.route_select_dual(og, hc, hf)
    o = oracle_mod.vq_assign_nchw(o_sel["h_dual"], E, o_sel["codebook_mask"])
    _check_routed(r, o_sel, o, B, oracle_mod)
    queued, listed = prep.fallback_count()
    print("routed dual K=%d B=%d: queued %d listed %d" % (K, B, queued, listed))
    assert listed == 0 and 0 <= queued < B * 1024


@pytest.mark.parametrize("B", [2, 10])
@pytest.mark.parametrize("K", KS)
def test_routed_triple(dev, oracle_mod, K, B):
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_triple
    D = 256
    E = synth.codebook_trained(K, D, seed=1300 + K)
    hf, hm, hco = (synth.z_tokens(E, B, 32, 32, 1310 + K), synth.z_tokens(E, B, 16, 16, 1320 + K),
                   synth.z_tokens(E, B, 8, 8, 1330 + K))
    lg = synth.grain_logits_triple(1340 + K, B, 8, 8)
    t = _t(dev)
    prep = _CodebookPrep()
    r = vq_assign_routed_triple(t(hco), t(hm), t(hf), t(E), prep, t(lg))
    o_sel = oracle_mod.route_select_triple(lg, hco, hm, hf)
    o = oracle_mod.vq_assign_nchw(o_sel["h_triple"], E, o_sel["codebook_mask"])
    _check_routed(r, o_sel, o, B, oracle_mod)
    queued, listed = prep.fallback_count()
    print("routed triple K=%d B=%d: queued %d listed %d" % (K, B, queued, listed))
    assert listed == 0 and 0 <= queued < B * 1024


@pytest.mark.parametrize("D", [64, 128, 256])
@pytest.mark.parametrize("shape", [(3, 16, 16), (20, 32, 32)])      # 768 positions: split form; 20480: one workgroup per block
@pytest.mark.parametrize("K", KS)
def test_dense_and_row_major(dev, oracle_mod, K, shape, D):
    """NCHW (split / cached / plain) and the same tokens row-major (flat form, and its split form)"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign
    B, H, W = shape
    E = synth.codebook_trained(K, D, seed=1400 + K)
    z = synth.z_tokens(E, B, H, W, 1410 + K + D)
    m = np.where(synth.uniform(1420 + K, (B, 1, H, W)) < 0.5, 1.0, 0.25).astype(np.float32)
    o = oracle_mod.vq_assign_nchw(z, E, m)
    ol = oracle_mod.vq_loss(o["sqerr"], o["numel"], 0.25)
    t = _t(dev)
    prep = _CodebookPrep()
    zq, codes, loss = vq_assign(t(z), t(E), prep, t(m))
    assert np.array_equal(codes.cpu().numpy().reshape(B, -1), o["codes"]), "codes"
    assert np.array_equal(zq.cpu().numpy(), o["zq"]), "z_q"
    assert C.loss_close(float(loss[1]), ol), "loss"
    queued, listed = prep.fallback_count()
    print("dense K=%d D=%d %r: queued %d listed %d" % (K, D, shape, queued, listed))
    assert listed == 0 and 0 <= queued < B * H * W
    zr = np.ascontiguousarray(np.moveaxis(z.reshape(B, D, H * W), 1, 2).reshape(-1, D))
    zq2, codes2, loss2 = vq_assign(t(zr), t(E), _CodebookPrep(), t(m.reshape(-1)))
    assert np.array_equal(codes2.cpu().numpy().reshape(B, -1), o["codes"]), "codes (row-major)"
    assert np.array_equal(np.moveaxis(zq2.cpu().numpy().reshape(B, H * W, D), 1, 2).reshape(z.shape), o["zq"]), "z_q (row-major)"
    assert C.loss_close(float(loss2[1]), ol), "loss (row-major)"


@pytest.mark.parametrize("D", [64, 256])
def test_split_form_with_slices_larger_than_the_table(dev, oracle_mod, D):
    """K = 16384 at 768 tokens: 8 slices of 64 code tiles, more than the table holds -- the split form (NCHW and row-major) with the
    per-tile seed piece"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign
    K, B, H, W = 16384, 3, 16, 16
    E = synth.codebook_trained(K, D, seed=1600 + D)
    z = synth.z_tokens(E, B, H, W, 1610 + D)
    o = oracle_mod.vq_assign_nchw(z, E, None)
    ol = oracle_mod.vq_loss(o["sqerr"], o["numel"], 0.25)
    t = _t(dev)
    zq, codes, loss = vq_assign(t(z), t(E), _CodebookPrep())
    assert np.array_equal(codes.cpu().numpy().reshape(B, -1), o["codes"]), "codes"
    assert np.array_equal(zq.cpu().numpy(), o["zq"]), "z_q"
    assert C.loss_close(float(loss[1]), ol), "loss"
    zr = np.ascontiguousarray(np.moveaxis(z.reshape(B, D, H * W), 1, 2).reshape(-1, D))
    zq2, codes2, loss2 = vq_assign(t(zr), t(E), _CodebookPrep())
    assert np.array_equal(codes2.cpu().numpy().reshape(B, -1), o["codes"]), "codes (row-major)"
    assert np.array_equal(np.moveaxis(zq2.cpu().numpy().reshape(B, H * W, D), 1, 2).reshape(z.shape), o["zq"]), "z_q (row-major)"
    assert C.loss_close(float(loss2[1]), ol), "loss (row-major)"


@pytest.mark.parametrize("B", [2, 12])
@pytest.mark.parametrize("K", KS)
def test_conv_and_fold(dev, oracle_mod, K, B):
    """the model order (select -> 1x1 quant_conv -> assign) as one op: codes / z_q bit-exact vs the oracle GIVEN the conv output the
    kernel scored (h_buf), and the same op on the conv-folded codebook: the same codes, z_q = e[code]"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_dual
    D = 256
    E = synth.codebook_trained(K, D, seed=1500 + K)
    hf, hc = synth.z_tokens(E, B, 32, 32, 1510 + K), synth.z_tokens(E, B, 16, 16, 1520 + K)
    ent = synth.entropy_map(1530 + K, B, 16, 16)
    t = _t(dev)
    conv = torch.nn.Conv2d(D, D, 1).to(dev).eval()
    with torch.no_grad():
        conv.weight.copy_(t(synth.normal(1540, (D, D, 1, 1), 0.0, 1.0 / 16.0)))
        conv.bias.copy_(t(synth.normal(1541, (D,), 0.0, 0.1)))
        hb = torch.empty((B, D, 32, 32), device=dev)
        rc = vq_assign_routed_dual(t(hc), t(hf), t(E), _CodebookPrep(), entropy=t(ent), threshold=THR, conv=conv, h_buf=hb)
        rf = vq_assign_routed_dual(t(hc), t(hf), t(E), _CodebookPrep(), entropy=t(ent), threshold=THR, conv=conv, fold=True,
                                   want_loss=False)
    og = oracle_mod.entropy_gate(ent, THR)
    o_sel = oracle_mod.route_select_dual(og, hc, hf)
    h = hb.cpu().numpy()
    o = oracle_mod.vq_assign_nchw(h, E, o_sel["codebook_mask"])
    _check_routed(rc, o_sel, o, B, oracle_mod)
    assert np.array_equal(rf["indices"].cpu().numpy(), o_sel["indices"]) and rf["loss"] is None
    assert np.array_equal(rf["codes"].cpu().numpy().reshape(B, -1), o["codes"]), "codes (fold)"
    eq = np.moveaxis(E[o["codes"]], 2, 1).reshape(B, D, 32, 32)
    assert np.all(np.abs(rf["zq"].cpu().numpy() - eq) <= 1e-6 * np.maximum(1.0, np.abs(h))), "z_q (fold)"


def test_bench_step_queue_counts_equal_the_parents(dev, oracle_mod):
    """the bench step (routed dual op, B = 256, K = 1024, three-stream slot 0's inputs): every output against the oracle on all
    images, and the resolver queue's (queued, listed) equal to what the parent commit's pass 1 queued on the same inputs"""
    from dynamicvectorquantization_amd import synth
    from dynamicvectorquantization_amd.quantize import _CodebookPrep, vq_assign_routed_dual
    B, K, D, b0 = 256, 1024, 256, 128
    E = synth.codebook_trained(K, D)
    tile = lambda base: np.ascontiguousarray(np.concatenate([np.roll(base, 5 * j, axis=-1) for j in range(B // b0)], 0))
    hf, hc = tile(synth.z_tokens(E, b0, 32, 32, 2903)), tile(synth.z_tokens(E, b0, 16, 16, 2913))
    ent = tile(synth.entropy_map(5903, b0, 16, 16))
    t = _t(dev)
    prep = _CodebookPrep()
    r = vq_assign_routed_dual(t(hc), t(hf), t(E), prep, entropy=t(ent), threshold=THR)
    counts = tuple(int(v) for v in prep.fallback_count())
    print("bench step: queued %d listed %d" % counts)
    og = oracle_mod.entropy_gate(ent, THR)
    o_sel = oracle_mod.route_select_dual(og, hc, hf)
    o = oracle_mod.vq_assign_nchw(o_sel["h_dual"], E, o_sel["codebook_mask"])
    _check_routed(r, o_sel, o, B, oracle_mod)
    assert counts == PARENT_BENCH_FALLBACK
