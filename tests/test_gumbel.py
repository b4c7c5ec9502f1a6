"""GumbelQuantize (quantize.py) and its kernel (dvq_gumbel_prepare_f32, dvq_vq_gumbel_assign_f32) against the float64 restatement
tests/_gumbel_ref.py and the reference's own module on the CPU (tests/golden/gumbel_quantize_B2.npz, written by
tools/gen_golden_gumbel.py).

Bounds.  codes: equal wherever the float64 top-2 gap of the scores exceeds margin = 8 * err_ref (the fixture's meta; derived in
tests/_gumbel_ref.py), at most 2 % of a case's tokens left out.  KL: 1e-5 relative of the float64 value.  z_q: bit-equal to
E[code]; within 2^-22 relative of the reference's z_q."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import _gumbel_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dvq_gumbel_prep_bytes", "dvq_gumbel_prepare_f32", "dvq_vq_gumbel_assign_workspace_bytes", "dvq_vq_gumbel_assign_f32")
_CACHE = {}


def _golden():
    if "g" not in _CACHE:
        g = R.load()
        for a in g.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _CACHE["g"] = g
    return _CACHE["g"]


def _case(name):
    """inputs and the float64 results per tau (None: no noise), computed once and shared read-only"""
    if name not in _CACHE:
        inp = R.inputs(name, _golden())
        z, W, b, E, q = inp
        ref = {tau: R.forward(z, W, b, E, q, tau) for tau in R.TAUS}
        ref[None] = R.forward(z, W, b, E, None, 1.0)
        for arr in inp + tuple(a for r in ref.values() for a in r if isinstance(a, np.ndarray)):
            arr.setflags(write=False)
        _CACHE[name] = (inp, ref)
    return _CACHE[name]


def _margin():
    return float(_golden()["meta"]["margin"])


# ---------------------------------------------------------------------------------------------------------------- CPU

def test_symbols_declared_and_exported():
    """the feature is there: the class imports, the four entry points are declared in include/dvq.h, pass the version script
    (a `dvq_*` global pattern) into the dynamic symbol table, and are bound; ABI 0.13.0"""
    import subprocess
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import GumbelQuantize  # noqa: F401
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dvq.h")).read(), flags=re.S)
    raw = ctypes.CDLL(_lib.LIB_PATH)
    syms = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True).split()
    mapfile = open(os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "libdvq.map")).read()
    assert re.search(r"global:\s*dvq_\*;", mapfile)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(raw, name) and name in _lib.EXPORTS and name in syms
    assert _lib.lib.dvq_version() >= 1300


def test_abi_validation_without_gpu():
    from dynamicvectorquantization_amd import _lib
    L = _lib.lib
    EINVAL, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    a = 256                                                        # a "pointer" that passes the alignment checks

    def call(z=a, prep=a, embed=a, B=2, C=64, HW=36, K=200, d=16, tau=1.0, kl_K=200.0, q=0, zq=a, codes=a, kl=0, ws=0, wsb=0):
        return L.dvq_vq_gumbel_assign_f32(z, prep, embed, B, C, HW, K, d, tau, kl_K, q, zq, codes, kl, ws, wsb, 0)

    for null in ("z", "prep", "embed", "codes"):
        assert call(**{null: 0}) == EINVAL and b"null" in L.dvq_last_error_string()
    assert call(C=100) == EUNSUPPORTED
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert call(q=a, tau=bad) == EINVAL and b"tau" in L.dvq_last_error_string()
    for bad in (0.0, -3.0, float("nan")):
        assert call(kl_K=bad) == EINVAL and b"kl_K" in L.dvq_last_error_string()
    need = L.dvq_vq_gumbel_assign_workspace_bytes(2, 36)
    assert need >= 8 and L.dvq_vq_gumbel_assign_workspace_bytes(0, 36) == 0
    assert call(kl=a, ws=0, wsb=0) == EINVAL and b"workspace" in L.dvq_last_error_string()
    assert call(kl=a, ws=a, wsb=need - 1) == EINVAL
    assert call(d=0) == EINVAL and call(B=0) == EINVAL
    assert L.dvq_gumbel_prep_bytes(200, 64) >= 7 * (32 * 64 + 64) * 4 and L.dvq_gumbel_prep_bytes(200, 100) == 0
    assert L.dvq_gumbel_prepare_f32(a, 0, 200, 100, a, 1 << 30, 0) == EUNSUPPORTED
    assert L.dvq_gumbel_prepare_f32(0, 0, 200, 64, a, 1 << 30, 0) == EINVAL
    assert L.dvq_gumbel_prepare_f32(a, 0, 200, 64, a, 16, 0) == EWORKSPACE


@pytest.mark.parametrize("i", range(len(R.TAUS)))
def test_restatement_reproduces_the_reference(i):
    """tests/_gumbel_ref.py against the reference's ind / diff / z_q of the fixture, with the margin rule and the cap"""
    g = _golden()
    tau = R.TAUS[i]
    s, codes, kl, zq = _case("golden")[1][tau]
    keep = R.top2_gap(s) > _margin()
    assert 1.0 - keep.mean() <= R.SKIP_CAP
    ind = g["ind%d" % i]
    assert ind.dtype == np.int64 and ind.shape == codes.shape
    assert np.array_equal(codes[keep], ind[keep])
    want = float(g["diff%d" % i]) / g["meta"]["kl_weight"]
    assert abs(kl - want) <= 1e-5 * abs(want)
    same = np.broadcast_to((codes == ind)[:, None], zq.shape)
    assert (np.abs(zq - g["zq%d" % i])[same] <= 2.0 ** -22 * np.abs(g["zq%d" % i])[same]).all()


def test_state_dict_keys_and_cpu_tensors_raise():
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import GumbelQuantize
    g = _golden()
    m = GumbelQuantize(64, 16, 200)
    assert sorted(m.state_dict().keys()) == g["meta"]["state_keys"] == ["embed.weight", "proj.bias", "proj.weight"]
    sd = {"proj.weight": torch.from_numpy(g["W"].copy()).reshape(200, 64, 1, 1), "proj.bias": torch.from_numpy(g["b"].copy()),
          "embed.weight": torch.from_numpy(g["E"].copy())}
    m.load_state_dict(sd, strict=True)                             # a reference state_dict loads
    assert torch.equal(m.embed.weight.detach(), sd["embed.weight"])
    for mod in (m, m.eval()):
        with pytest.raises(_lib.DvqError):
            mod(torch.zeros(1, 64, 2, 2))
    idx = torch.tensor([3, 0, 199, 7])
    e = m.get_codebook_entry(idx, (1, 2, 2, 16))
    assert tuple(e.shape) == (1, 16, 2, 2) and torch.equal(e[0, :, 1, 0], m.embed.weight.detach()[199])


# ---------------------------------------------------------------------------------------------------------------- GPU

def _t(a, dev):
    return None if a is None else torch.tensor(np.ascontiguousarray(a), device=dev)


def _prep(W, b, dev):
    from dynamicvectorquantization_amd import _lib
    K, C = W.shape
    nb = _lib.lib.dvq_gumbel_prep_bytes(K, C)
    buf = torch.empty(nb, dtype=torch.uint8, device=dev)
    Wt, bt = _t(W, dev), _t(b, dev)
    _lib.check(_lib.lib.dvq_gumbel_prepare_f32(Wt.data_ptr(), _lib.ptr(bt), K, C, buf.data_ptr(), nb, _lib.stream_ptr(dev)), "prepare")
    return buf


def _check_against(ref, got, E):
    """(zq, codes, kl) of the kernel against forward()'s (s, codes, kl, zq) -> the kernel's codes as numpy"""
    s, codes, kl, _ = ref
    zq, ind, klv = got
    assert ind.dtype == torch.int64 and tuple(ind.shape) == codes.shape
    ind = ind.cpu().numpy()
    keep = R.top2_gap(s) > _margin()
    left = 1.0 - float(keep.mean())
    print("left out %.5f  KL %.8f (float64 %.8f)" % (left, float(klv), kl))
    assert left <= R.SKIP_CAP
    assert np.array_equal(ind[keep], codes[keep])
    assert abs(float(klv) - kl) <= 1e-5 * abs(kl)
    assert np.array_equal(zq.cpu().numpy(), E[ind].transpose(0, 3, 1, 2))      # bit-equal to the codebook rows
    return ind


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(R.CASES))
def test_kernel_parity_with_noise(name, dev):
    from dynamicvectorquantization_amd.quantize import gumbel_assign
    (z, W, b, E, q), ref = _case(name)
    g = _golden()
    prep, zt, Et, qt = _prep(W, b, dev), _t(z, dev), _t(E, dev), _t(q, dev)
    for i, tau in enumerate(R.TAUS):
        got = gumbel_assign(zt, prep, Et, tau, qt)
        ind = _check_against(ref[tau], got, E)
        if name == "golden":                                       # the reference's own z_q and ind
            rz, ri = g["zq%d" % i], g["ind%d" % i]
            same = np.broadcast_to((ind == ri)[:, None], rz.shape)
            assert same.mean() >= 1.0 - R.SKIP_CAP
            assert (np.abs(got[0].cpu().numpy() - rz)[same] <= 2.0 ** -22 * np.abs(rz)[same]).all()
    if name == "flat":                                             # the same tokens as [N, C]: HW == 1 with two dims
        got2 = gumbel_assign(zt.reshape(z.shape[0], z.shape[1]), prep, Et, R.TAUS[0], qt)
        ref_got = gumbel_assign(zt, prep, Et, R.TAUS[0], qt)
        assert torch.equal(got2[1], ref_got[1].reshape(-1)) and torch.equal(got2[2], ref_got[2])
    again = gumbel_assign(zt, prep, Et, R.TAUS[0], qt)             # deterministic: the same bits run to run
    first = gumbel_assign(zt, prep, Et, R.TAUS[0], qt)
    assert torch.equal(again[2], first[2]) and torch.equal(again[1], first[1])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["golden", "odd"])
def test_kernel_without_noise_is_the_argmax_of_the_logits(name, dev):
    from dynamicvectorquantization_amd.quantize import gumbel_assign
    (z, W, b, E, q), ref = _case(name)
    prep = _prep(W, b, dev)
    got = gumbel_assign(_t(z, dev), prep, _t(E, dev), 0.0, None)   # tau is ignored without q
    _check_against(ref[None], got, E)
    only = gumbel_assign(_t(z, dev), prep, _t(E, dev), 1.0, None, want_zq=False, want_kl=False)
    assert only[0] is None and only[2] is None and torch.equal(only[1], got[1])
    nob = gumbel_assign(_t(z, dev), _prep(W, None, dev), _t(E, dev), 1.0, None)       # a conv without bias
    _check_against(R.forward(z, W, np.zeros_like(b), E, None, 1.0), nob, E)


@pytest.mark.gpu
def test_special_values(dev):
    """a NaN logit wins and the first NaN wins; equal logits with equal noise give the first index"""
    from dynamicvectorquantization_amd.quantize import gumbel_assign
    (z, W, b, E, q), _ = _case("golden")
    zt, Et, qt = _t(z, dev), _t(E, dev), _t(q, dev)
    bn = b.copy()
    bn[[150, 37, 101]] = np.nan                                    # three NaN logits per token, in tiles 4, 1, 3
    for qq in (None, qt):
        zq, ind, kl = gumbel_assign(zt, _prep(W, bn, dev), Et, 1.0, qq)
        assert bool((ind == 37).all()) and bool(torch.isnan(kl).all())
        assert torch.equal(zq[1, :, 2, 3], Et[37])
    zn = z.copy()
    zn[1, 5, 0, 4] = np.nan                                        # every logit of one token NaN: index 0
    _, ind, _ = gumbel_assign(_t(zn, dev), _prep(W, b, dev), Et, 1.0, qt)
    assert int(ind[1, 0, 4]) == 0
    Wd, bd = W.copy(), b.copy()
    Wd[:] = W[11]                                                  # every code the same logit ...
    bd[:] = 0.25
    qc = torch.full_like(qt, 0.7)                                  # ... and the same noise: the first index
    for qq in (None, qc):
        _, ind, kl = gumbel_assign(zt, _prep(Wd, bd, dev), Et, 0.5, qq)
        assert bool((ind == 0).all())
        assert abs(float(kl)) <= 1e-6                              # the uniform distribution: KL = 0
    bd[[133, 40, 199]] = 5.0                                       # three equal maxima: the first of them
    _, ind, _ = gumbel_assign(zt, _prep(Wd, bd, dev), Et, 0.5, qc)
    assert bool((ind == 40).all())


def _module(dev, name="golden", **kw):
    from dynamicvectorquantization_amd.quantize import GumbelQuantize
    B, C, H, Wd, K, d, _ = R.CASES[name]
    z, W, b, E, q = _case(name)[0]
    m = GumbelQuantize(C, d, K, **kw)
    m.load_state_dict({"proj.weight": torch.from_numpy(W.copy()).reshape(K, C, 1, 1), "proj.bias": torch.from_numpy(b.copy()),
                       "embed.weight": torch.from_numpy(E.copy())}, strict="remap" not in kw)     # (remap adds the buffer `used`)
    return m.to(dev)


@pytest.mark.gpu
def test_module_fused_forward_matches_the_reference(dev):
    (z, W, b, E, q), ref = _case("golden")
    g = _golden()
    m = _module(dev).eval()
    for i, tau in enumerate(R.TAUS):
        with torch.no_grad():
            zq, diff, (a0, a1, ind) = m(_t(z, dev), temp=tau, q=_t(q, dev))
        assert m.last_path == "fused" and a0 is None and a1 is None and diff.dim() == 0
        _check_against(ref[tau], (zq, ind, diff / m.kl_weight), E)
        ri = g["ind%d" % i]
        assert ind.dtype == torch.int64 and tuple(ind.shape) == ri.shape
        # the reference's fp32 diff is within 1e-5 of the float64 value (asserted by the generator), the kernel's too
        assert abs(float(diff) - float(g["diff%d" % i])) <= 2e-5 * abs(float(g["diff%d" % i]))
    m.use_vqinterface = False
    with torch.no_grad():
        out = m(_t(z, dev), temp=R.TAUS[-1], q=_t(q, dev))
    assert len(out) == 3 and torch.equal(out[2], ind)


@pytest.mark.gpu
def test_module_prepared_image_follows_in_place_edits(dev):
    (z, W, b, E, q), _ = _case("golden")
    m = _module(dev).eval()
    zt, qt = _t(z, dev), _t(q, dev)
    with torch.no_grad():
        m(zt, q=qt)
        buf0 = m._proj_img.buf
        m(zt, q=qt)
        assert m._proj_img.buf is buf0                             # steady state: no rebuild
        m.proj.weight.mul_(-1.0)
        _, _, (_, _, ind) = m(zt, q=qt)
        s, codes, _, _ = R.forward(z, -W, b, E, q, 1.0)
        keep = R.top2_gap(s) > _margin()
        assert keep.mean() >= 1.0 - R.SKIP_CAP and np.array_equal(ind.cpu().numpy()[keep], codes[keep])
        assert not np.array_equal(codes, _case("golden")[1][1.0][1])
        m.proj.bias[123] += 100.0
        _, _, (_, _, ind) = m(zt, q=qt)
        assert bool((ind == 123).all())
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        sd["proj.bias"][123] -= 100.0
        sd["proj.bias"][7] += 100.0
        m.load_state_dict(sd)
        assert bool((m(zt, q=qt)[2][2] == 7).all())


@pytest.mark.gpu
def test_module_seeding_follows_torch(dev):
    """forward consumes torch's generator exactly as torch.empty(B, K, H, W).exponential_() does"""
    (z, W, b, E, q), _ = _case("golden")
    B, C, H, Wd, K, d, _ = R.CASES["golden"]
    m = _module(dev).eval()
    zt = _t(z, dev)
    with torch.no_grad():
        torch.manual_seed(1234)
        _, d1, (_, _, i1) = m(zt)
        s1 = torch.cuda.get_rng_state(dev)
        torch.manual_seed(1234)
        _, d2, (_, _, i2) = m(zt)
        torch.manual_seed(1234)
        qq = torch.empty(B, K, H, Wd, device=dev).exponential_()
        s3 = torch.cuda.get_rng_state(dev)
        _, d3, (_, _, i3) = m(zt, q=qq)
    assert m.last_path == "fused"
    assert torch.equal(i1, i2) and torch.equal(i1, i3) and torch.equal(d1, d2) and torch.equal(d1, d3)
    assert torch.equal(s1, s3)


@pytest.mark.gpu
def test_module_routing_and_gradients(dev, tmp_path):
    (z, W, b, E, q), ref = _case("golden")
    B, C, H, Wd, K, d, _ = R.CASES["golden"]
    zt, qt = _t(z, dev), _t(q, dev)
    # grad enabled: the torch path, gradients to proj, embed and z equal to the same expression written inline
    m = _module(dev).train()
    zg = zt.clone().requires_grad_(True)
    zq, diff, (_, _, ind) = m(zg, temp=0.5, q=qt)
    assert m.last_path == "torch" and zq.requires_grad
    wsum = torch.linspace(-1.0, 1.0, zq.numel(), device=dev).reshape(zq.shape)
    ((zq * wsum).sum() + diff).backward()
    got = [zg.grad.clone(), m.proj.weight.grad.clone(), m.proj.bias.grad.clone(), m.embed.weight.grad.clone()]
    m2 = _module(dev).train()
    z2 = zt.clone().requires_grad_(True)
    logits = torch.nn.functional.conv2d(z2, m2.proj.weight, m2.proj.bias)
    y = ((logits - qt.log()) / 0.5).softmax(1)
    hard_ = torch.zeros_like(y).scatter_(1, y.max(1, keepdim=True)[1], 1.0) - y.detach() + y
    zq2 = torch.einsum('b n h w, n d -> b d h w', hard_, m2.embed.weight)
    p = logits.softmax(1)
    diff2 = m2.kl_weight * torch.sum(p * torch.log(p * K + 1e-10), dim=1).mean()
    ((zq2 * wsum).sum() + diff2).backward()
    want = [z2.grad, m2.proj.weight.grad, m2.proj.bias.grad, m2.embed.weight.grad]
    assert torch.equal(ind, hard_.argmax(1)) and torch.allclose(zq, zq2) and torch.allclose(diff, diff2)
    for a_, b_ in zip(got, want):
        assert a_ is not None and float(a_.abs().max()) > 0 and torch.allclose(a_, b_)
    keep = R.top2_gap(ref[0.5][0]) > _margin()
    assert np.array_equal(ind.cpu().numpy()[keep], ref[0.5][1][keep])
    # no_grad, training, soft (straight_through=False): the torch path; eval forces hard = True: the fused path
    ms = _module(dev, straight_through=False).train()
    with torch.no_grad():
        zs, _, _ = ms(zt, q=qt)
        assert ms.last_path == "torch"
        ze, _, (_, _, ie) = ms.eval()(zt, q=qt)
        assert ms.last_path == "fused" and torch.equal(ze, ms.embed.weight[ie].permute(0, 3, 1, 2))
        assert not torch.equal(zs, ze)                             # the soft mixture is not a codebook row
        # training with straight_through=True under no_grad: hard, fused
        _module(dev).train()(zt, q=qt)
        # return_logits: the torch path, the logits as the fourth result
        me = _module(dev).eval()
        out = me(zt, q=qt, return_logits=True)
        assert me.last_path == "torch" and len(out) == 4 and tuple(out[3].shape) == (B, K, H, Wd)
        assert torch.equal(out[2][2], ie)
        # remap: the torch path
        used = np.arange(0, K, 2)
        np.save(tmp_path / "used.npy", used)
        mr = _module(dev, remap=str(tmp_path / "used.npy"), unknown_index="extra").eval()
        zr, _, (_, _, ir) = mr(zt, q=qt[:, ::2].contiguous())
        assert mr.last_path == "torch" and tuple(ir.shape) == (B, H, Wd) and int(ir.max()) < len(used)
        assert torch.allclose(zr, mr.embed.weight[2 * ir].permute(0, 3, 1, 2), rtol=2.0 ** -22, atol=0)
    # another width: the torch path on the GPU, not a raise
    from dynamicvectorquantization_amd.quantize import GumbelQuantize
    mo = GumbelQuantize(100, 8, 32).to(dev).eval()
    with torch.no_grad():
        zo, do, (_, _, io) = mo(torch.randn(2, 100, 3, 3, device=dev))
    assert mo.last_path == "torch" and tuple(zo.shape) == (2, 8, 3, 3) and tuple(io.shape) == (2, 3, 3)
    assert torch.allclose(zo, mo.embed.weight[io].permute(0, 3, 1, 2), rtol=2.0 ** -22, atol=0)


@pytest.mark.gpu
def test_graph_capture(dev):
    """the fused call with preallocated outputs captures into a graph (a single chain) and replays on new inputs"""
    from dynamicvectorquantization_amd import _lib
    from dynamicvectorquantization_amd.quantize import gumbel_assign
    (z, W, b, E, q), _ = _case("golden")
    B, C, H, Wd, K, d, _ = R.CASES["golden"]
    prep, zt, Et, qt = _prep(W, b, dev), _t(z, dev), _t(E, dev), _t(q, dev)
    out = (torch.empty(B, d, H, Wd, device=dev), torch.empty(B, H, Wd, dtype=torch.int64, device=dev), torch.empty(1, device=dev),
           torch.empty(_lib.lib.dvq_vq_gumbel_assign_workspace_bytes(B, H * Wd), dtype=torch.uint8, device=dev))
    step = lambda: gumbel_assign(zt, prep, Et, 0.5, qt, out=out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    zt.copy_(torch.flip(zt, dims=(0, 2)))
    qt.copy_(torch.flip(qt, dims=(3,)))
    graph.replay()
    torch.cuda.synchronize()
    got = [o.clone() for o in out[:3]]
    want = gumbel_assign(zt, prep, Et, 0.5, qt)
    for a_, b_ in zip(got, want):
        assert torch.equal(a_, b_)
