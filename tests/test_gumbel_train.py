"""GumbelQuantize's training step on the GPU: the forward that keeps the logits (vq_gumbel_assign_kernel<D, NOISE, true>,
quantize.gumbel_forward_train), the backward kernel (csrc/vq_gumbel_backward.hip, quantize.gumbel_backward_logits) and the module
with `fused_backward` on (quantize.gumbel_quantize, GumbelQuantizeFused).

Cases: tests/_score_cases.GUMBEL_CASES -- K = 1 .. 160 (K <= 4: code slices without a code), N = 1 .. 32 897 (the backward's
16-wave form below 1024 workgroups of 32 tokens, its 4-wave form from there: `n-32897x64` is 1029), with and without q, tau 1.0 and
0.5, bias ramps, logits of standard deviation 30, -inf on 40 codes / all but one / all codes.  That table stays within one chunk of
the backward's per-lane code loop; tests/_gumbel_train_ref.CHUNK_CASES (K = 600 and 1100 in the 16-wave form, K = 264 at 33 825 tokens
in the 4-wave form) run it over several.  Reference, mixes and bound:
tests/_gumbel_train_ref.py (float64; max |dl - dl64| <= 1.9e-5 max |dl64|, 8 x the float32 torch chain's own error, which
tests/test_gumbel_train_cases.py measures).  The observed error is printed per case and mix."""
import numpy as np
import pytest
import torch

from tests import _gumbel_ref as GR
from tests import _gumbel_train_ref as T
from tests import _score_cases as C

NAMES = [c.name for c in C.GUMBEL_CASES]


def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _off4(t):
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    buf[1:].copy_(t.reshape(-1))
    return buf[1:].view(t.shape)


def _prep(W, b, dev):
    from dynamicvectorquantization_amd import _lib
    K, Cc = W.shape
    nb = _lib.lib.dvq_gumbel_prep_bytes(K, Cc)
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    Wt, bt = _t(W, dev), _t(b, dev)
    _lib.check(_lib.lib.dvq_gumbel_prepare_f32(Wt.data_ptr(), _lib.ptr(bt), K, Cc, buf.data_ptr(), nb, _lib.stream_ptr(dev)), "prepare")
    return buf


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---------------------------------------------------------------- 1. the forward ------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_forward_train_is_the_sweep_and_keeps_its_logits(name, dev, oracle_mod):
    from dynamicvectorquantization_amd.quantize import gumbel_assign, gumbel_forward_train
    c = C.G_BY_NAME[name]
    inp = C.gumbel_inputs(c, oracle_mod)
    Et = _t(inp["E"], dev)
    if c.e_offset:
        Et = _off4(Et)
    z, prep, q = _t(inp["z"], dev), _prep(inp["W"], inp["b"], dev), _t(inp["q"], dev)
    zq0, codes0, kl0 = gumbel_assign(z, prep, Et, c.tau, q, kl_K=c.kl_K)
    zq, codes, kl, logits = gumbel_forward_train(z, prep, Et, c.tau, q, kl_K=c.kl_K)
    assert torch.equal(codes, codes0) and torch.equal(_bits(zq), _bits(zq0)) and torch.equal(_bits(kl), _bits(kl0))
    assert tuple(logits.shape) == T.logits_shape(c)
    want = C.to_layout(inp["l32"], T.logits_shape(c))
    assert np.array_equal(logits.cpu().numpy().view(np.uint32), want.view(np.uint32))       # NaN / inf patterns included


# ---------------------------------------------------------------- 2. the backward kernel ----------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_backward_kernel_against_float64(name, dev, oracle_mod):
    from dynamicvectorquantization_amd.quantize import gumbel_backward_logits
    c = C.G_BY_NAME[name]
    inp, tr = C.gumbel_inputs(c, oracle_mod), T.train_inputs(c, oracle_mod)
    shape = T.logits_shape(c)
    logits, q, u = _t(C.to_layout(inp["l32"], shape), dev), _t(inp["q"], dev), _t(C.to_layout(tr["u32"], shape), dev)
    dead = ~np.isfinite(inp["b"])
    for mix, with_u, g_kl in T.MIXES:
        g = None if g_kl is None else torch.tensor([g_kl], dtype=torch.float32, device=dev)
        out = torch.full(shape, 7.0, dtype=torch.float32, device=dev)
        got_t = gumbel_backward_logits(logits, q, u if with_u else None, g, c.tau, inp["kl_K"], out=out)
        assert got_t is out
        got = C.to_rows(out.cpu().numpy())
        want = tr[mix]
        err, same_nan = T.error(got, want, tr["u32"] if with_u else None, c.tau)
        print("%s %s: max |dl - dl64| / scale %.3g" % (name, mix, err))
        assert same_nan, (name, mix)
        assert err <= T.BOUND, (name, mix, err)
        if c.bias == "allinf":
            assert np.isnan(got).all()
        elif dead.any():
            assert not got[:, dead].any()                                # codes at -inf: exactly 0
        again = gumbel_backward_logits(logits, q, u if with_u else None, g, c.tau, inp["kl_K"], out=torch.empty_like(out))
        assert torch.equal(_bits(again), _bits(out))                     # the same bits run to run
        if with_u:
            over = u.clone()
            res = gumbel_backward_logits(logits, q, over, g, c.tau, inp["kl_K"])
            assert res is over and torch.equal(_bits(over), _bits(out))  # dlogits aliased to u


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in T.CHUNK_CASES])
def test_backward_kernel_over_several_chunks(name, dev):
    """K of several chunks of the lane's code loop, in both forms of the kernel (tests/_gumbel_train_ref.CHUNK_CASES): the running
    rescale when a later chunk raises the maximum, the sums across chunks, a first chunk without a finite value, pass B's later
    iterations.  Logits, q and u go straight to the kernel; the reference is dl64 on the same arrays"""
    from dynamicvectorquantization_amd.quantize import gumbel_backward_logits
    c = T.CHUNK_BY_NAME[name]
    inp = T.chunk_inputs(c)
    shape = (c.B, c.K, c.HW)
    logits, u = _t(C.to_layout(inp["l32"], shape), dev), _t(C.to_layout(inp["u32"], shape), dev)
    q = None if inp["qrows"] is None else _t(C.to_layout(inp["qrows"], shape), dev)
    for mix, with_u, g_kl in T.MIXES:
        g = None if g_kl is None else torch.tensor([g_kl], dtype=torch.float32, device=dev)
        out = torch.full(shape, 7.0, dtype=torch.float32, device=dev)
        gumbel_backward_logits(logits, q, u if with_u else None, g, c.tau, inp["kl_K"], out=out)
        got = C.to_rows(out.cpu().numpy())
        err, same_nan = T.error(got, inp[mix], inp["u32"] if with_u else None, c.tau)
        print("%s %s: max |dl - dl64| / scale %.3g" % (name, mix, err))
        assert same_nan, (name, mix)
        assert err <= T.BOUND, (name, mix, err)
        if c.kind == "inf_lead":
            assert np.isnan(got[list(T.CHUNK_NAN_ROWS)]).all()
            rest = np.delete(got, T.CHUNK_NAN_ROWS, axis=0)
            assert inp["dead"].sum() == c.lead and not rest[:, inp["dead"]].any()        # codes at -inf: exactly 0
        if with_u:
            over = u.clone()
            assert gumbel_backward_logits(logits, q, over, g, c.tau, inp["kl_K"]) is over and torch.equal(_bits(over), _bits(out))


@pytest.mark.gpu
def test_backward_rejects_a_wrong_out(dev):
    from dynamicvectorquantization_amd.quantize import gumbel_backward_logits
    logits = torch.zeros(2, 5, 3, device=dev)
    g = torch.ones(1, device=dev)
    for bad in (torch.empty(2, 5, 2, device=dev), torch.empty(2, 5, 3, device=dev, dtype=torch.float64), torch.empty(2, 5, 3),
                torch.empty(2, 3, 5, device=dev).transpose(1, 2)):
        with pytest.raises(ValueError, match="out must be"):
            gumbel_backward_logits(logits, None, None, g, 1.0, out=bad)


@pytest.mark.gpu
def test_backward_kernel_without_any_gradient_writes_zeros(dev, oracle_mod):
    from dynamicvectorquantization_amd.quantize import gumbel_backward_logits
    c = C.G_BY_NAME["kl-allinf"]
    inp = C.gumbel_inputs(c, oracle_mod)
    shape = T.logits_shape(c)
    out = torch.full(shape, 7.0, dtype=torch.float32, device=dev)
    gumbel_backward_logits(_t(C.to_layout(inp["l32"], shape), dev), _t(inp["q"], dev), None, None, c.tau, out=out)
    assert not out.any()


# ---------------------------------------------------------------- 3. the module --------------------------------------------------
G_KL = 0.35


def _module(cls, dev, W, b, E, **kw):
    K, Cc = W.shape
    m = cls(Cc, E.shape[1], K, **kw).to(dev)
    with torch.no_grad():
        m.proj.weight.copy_(_t(W, dev).view(K, Cc, 1, 1))
        m.proj.bias.copy_(_t(b, dev))
        m.embed.weight.copy_(_t(E, dev))
    return m


def _step(m, z, q, G, z_grad=True):
    """one training step: -> (z_q, diff, ind, [dz, dW, db, dE]) with loss = sum(z_q G) + (G_KL / kl_weight) diff"""
    for p in m.parameters():
        p.grad = None
    zt = z.clone().requires_grad_(z_grad)
    z_q, diff, (_, _, ind) = m(zt, q=q)
    torch.autograd.backward([z_q, diff], [G, torch.tensor(G_KL / m.kl_weight, device=z.device)])
    return z_q.detach(), diff.detach(), ind, [zt.grad, m.proj.weight.grad, m.proj.bias.grad, m.embed.weight.grad]


def _errors(grads, want):
    out = []
    for g, w in zip(grads, want):
        g = g.detach().double().cpu().numpy().reshape(w.shape)
        out.append(float(np.abs(g - w).max() / np.abs(w).max()))
    return out


@pytest.mark.gpu
def test_module_trains_on_the_kernels(dev):
    from dynamicvectorquantization_amd.quantize import GumbelQuantize
    z, W, b, E, q = GR.inputs("golden", GR.load())
    zt, qt = _t(z, dev), _t(q, dev)
    rng = np.random.default_rng(9191)
    G = rng.standard_normal((z.shape[0], E.shape[1]) + z.shape[2:]).astype(np.float32)
    Gt = _t(G, dev)
    m = _module(GumbelQuantize, dev, W, b, E)
    assert m.fused_backward is False
    m.eval()
    with torch.no_grad():
        zq_e, diff_e, (_, _, ind_e) = m(zt, q=qt)
    assert m.last_path == "fused"
    m.train()
    m.fused_backward = True
    zq_f, diff_f, ind_f, grads_f = _step(m, zt, qt, Gt)
    assert m.last_path == "fused_train"
    assert torch.equal(_bits(zq_f), _bits(zq_e)) and torch.equal(_bits(diff_f), _bits(diff_e)) and torch.equal(ind_f, ind_e)
    want = T.grads64(z, W, b, E, q, m.temperature, m.n_embed, ind_f.cpu().numpy(), G, G_KL)
    m.fused_backward = False
    _, _, ind_t, grads_t = _step(m, zt, qt, Gt)
    assert m.last_path == "torch"
    err_f, err_t = _errors(grads_f, want), _errors(grads_t, want)
    print("fused %s, torch ops %s (z, proj.weight, proj.bias, embed.weight)" % (err_f, err_t))
    for ef, et in zip(err_f, err_t):
        assert ef <= 8 * max(et, 1e-6), (err_f, err_t)
    # a channels_last gradient from the decoder
    m.fused_backward = True
    _, _, _, grads_cl = _step(m, zt, qt, Gt.contiguous(memory_format=torch.channels_last))
    assert m.last_path == "fused_train"
    err_cl = _errors(grads_cl, want)
    print("channels_last G: %s" % err_cl)
    for ec, et in zip(err_cl, err_t):
        assert ec <= 8 * max(et, 1e-6), (err_cl, err_t)
    # a z that needs no gradient gets none; the others are what they were
    _, _, _, grads_nz = _step(m, zt, qt, Gt, z_grad=False)
    assert m.last_path == "fused_train" and grads_nz[0] is None
    for en, et in zip(_errors(grads_nz[1:], want[1:]), err_t[1:]):
        assert en <= 8 * max(et, 1e-6)


@pytest.mark.gpu
def test_fused_class_checkpoints_and_the_paths_that_stay(dev, tmp_path):
    from dynamicvectorquantization_amd.quantize import GumbelQuantize, GumbelQuantizeFused
    z, W, b, E, q = GR.inputs("golden", GR.load())
    zt, qt = _t(z, dev), _t(q, dev)
    plain, fused = _module(GumbelQuantize, dev, W, b, E), GumbelQuantizeFused(W.shape[1], E.shape[1], W.shape[0]).to(dev)
    assert GumbelQuantizeFused.fused_backward is True and GumbelQuantize.fused_backward is False
    assert list(fused.state_dict()) == list(plain.state_dict())
    fused.load_state_dict(plain.state_dict())
    back = GumbelQuantize(W.shape[1], E.shape[1], W.shape[0]).to(dev)
    back.load_state_dict(fused.state_dict())
    for k, v in plain.state_dict().items():
        assert torch.equal(v, fused.state_dict()[k]) and torch.equal(v, back.state_dict()[k])
    fused.train()
    z_q, diff, _ = fused(zt.clone().requires_grad_(True), q=qt)
    assert fused.last_path == "fused_train" and z_q.requires_grad and diff.requires_grad
    # with the flag on, everything else goes where it went
    with torch.no_grad():
        fused(zt, q=qt)
    assert fused.last_path == "fused"
    fused(zt, q=qt, return_logits=True)
    assert fused.last_path == "torch"
    soft = _module(GumbelQuantizeFused, dev, W, b, E, straight_through=False).train()
    soft(zt, q=qt)
    assert soft.last_path == "torch"
    soft.eval()                                                         # eval forces the hard form: recorded autograd trains it
    soft(zt.clone().requires_grad_(True), q=qt)
    assert soft.last_path == "fused_train"
    used = tmp_path / "used.npy"
    np.save(used, np.arange(0, W.shape[0], 2))
    remapped = GumbelQuantizeFused(W.shape[1], E.shape[1], W.shape[0], remap=str(used)).to(dev).train()
    remapped(zt)
    assert remapped.last_path == "torch"
    narrow = GumbelQuantizeFused(32, 8, 40).to(dev).train()
    narrow(torch.randn(2, 32, 3, 3, device=dev))
    assert narrow.last_path == "torch"
