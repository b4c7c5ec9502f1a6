"""Residual quantization (dynamicvectorquantization_amd.rq.RQBottleneck, dvq_rq_*) at the reference's geometries: square code
grids, divisors 1 x 1 and 2 x 2, Dl a multiple of 4, depth 2 to 4.  tests/test_rq_shapes.py covers the other geometries, the depth
limits and the ABI with given codes; the restatement both files use is tests/_rq_ref.py.
CPU: the reference goldens (tests/golden/rq_*.npz, tools/gen_golden_rq.py) against a per-depth restatement built from the oracle's
assign and the float32 residual update -- which pins the restatement the GPU tests use at larger sizes --, constructor errors,
state_dict keys, ABI argument checks without a device.
GPU: goldens in both assign modes (codes exact; out, agg and embed_* equal as bit patterns, so the sign of zero counts; loss
1e-5), one training step (x.grad 1e-6, EMA buffers 1e-5), the reference RQ-VAE shape against the restatement, determinism, graph
capture, errors."""
import ctypes
import os

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib, synth
from dynamicvectorquantization_amd.rq import RQBottleneck
from tests._rq_ref import _books, _module, _restate, _to_latent, same_bits

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EVAL_CASES = ("eval_shared", "eval_separate")
TRAIN_CASES = ("train_shared", "train_separate")
ALL_CASES = EVAL_CASES + TRAIN_CASES


def _load(tag):
    return dict(np.load(os.path.join(GOLDEN, "rq_%s.npz" % tag)))


# ---- CPU --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tag", EVAL_CASES)
def test_golden_matches_oracle_restatement(oracle_mod, tag):
    rec = _load(tag)
    rH, rW = int(rec["latent_shape"][0] // rec["code_shape"][0]), int(rec["latent_shape"][1] // rec["code_shape"][1])
    codes, out, agg, loss = _restate(oracle_mod, rec["x"], _books(rec, int(rec["code_shape"][2])), rH, rW)
    assert np.array_equal(codes, rec["codes"])
    assert same_bits(out, rec["out"]) and same_bits(agg, rec["agg"])
    assert abs(loss - float(rec["loss"])) <= 1e-5 * abs(float(rec["loss"]))
    assert bool(rec["agg_equals_embed_code"]) and bool(rec["add_last_equals_embed_code"])


def test_constructor_errors_and_state_dict_keys():
    with pytest.raises(ValueError):
        RQBottleneck((8, 8), (8, 8, 4), 16)
    with pytest.raises(ValueError):
        RQBottleneck((8, 8, 64), (3, 8, 4), 16)
    with pytest.raises(ValueError):
        RQBottleneck((8, 8, 64), (8, 8, 2), [16, 16], shared_codebook=True)
    with pytest.raises(ValueError):
        RQBottleneck((8, 8, 64), (8, 8, 2), 16, decay=[0.9, 0.9], shared_codebook=True)
    for tag in ALL_CASES:
        rec = _load(tag)
        rq = _module(rec)
        assert list(rq.state_dict().keys()) == [str(k) for k in rec["state_dict_keys"]], tag
        assert tuple(rq.latent_shape) == tuple(rec["latent_shape"]) and tuple(rq.code_shape) == tuple(rec["code_shape"])
        assert list(rq.n_embed) == [int(k) for k in rec["n_embed"]]
        assert len(rq.shape_divisor) == 3 and len(rq.decay) == rq.code_shape[-1]
        assert (rq.codebooks[0] is rq.codebooks[-1]) == bool(rec["shared"])
    with pytest.raises(_lib.DvqError):                          # no CPU fallback
        _module(_load("eval_shared"))(torch.zeros(1, 8, 8, 256))


def test_abi_rejects_bad_arguments_without_a_device():
    L = _lib.lib
    fake = 1 << 20                                           # never dereferenced: every call below fails validation
    vp = ctypes.c_void_p

    def step(**kw):
        a = dict(x=fake, r=fake, E=fake, K=64, code=fake, B=1, h=8, w=8, rH=1, rW=1, Dl=256, D=256, i=0, depth=4, grad=0,
                 codes=fake, out=fake, ws=fake, ws_bytes=1 << 30)
        a.update(kw)
        return L.dvq_rq_step_f32(*[a[k] for k in ("x", "r", "E", "K", "code", "B", "h", "w", "rH", "rW", "Dl", "D", "i", "depth",
                                                   "grad", "codes", "out", "ws", "ws_bytes")], None)

    assert step(x=None) == -1 and step(code=None) == -1 and step(ws=None) == -1
    assert step(B=0) == -1 and step(K=0) == -1
    assert step(depth=_lib.RQ_MAX_DEPTH + 1) == -1 and step(i=4) == -1
    assert step(Dl=128) == -1                                # Dl rH rW != D
    assert step(ws=fake + 16) == -1                          # misaligned workspace
    assert step(Dl=48, D=48) == -2 and step(Dl=512, D=512) == -2
    assert step(ws_bytes=16) == -3
    assert L.dvq_rq_workspace_bytes(1024, 256, 4, 1) > L.dvq_rq_workspace_bytes(1024, 256, 4, 0) > 0
    assert L.dvq_rq_workspace_bytes(1024, 48, 4, 0) == 0 and L.dvq_rq_workspace_bytes(1024, 256, 17, 0) == 0
    o1, o2, o3 = (L.dvq_rq_residual_offset(1024, 256, 4, i) for i in (1, 2, 3))
    assert o1 % 256 == 0 and o2 - o1 >= 1024 * 256 * 4 and o3 == o1
    assert L.dvq_rq_residual_offset(1024, 256, 4, 0) == 0 and L.dvq_rq_residual_offset(1024, 256, 4, 4) == 0
    assert L.dvq_rq_loss_f32(1024, 256, 4, None, 1 << 30, fake, None) == -1
    assert L.dvq_rq_loss_f32(1024, 256, 0, fake, 1 << 30, fake, None) == -1
    assert L.dvq_rq_backward_f32(fake, fake, 1, 8, 8, 1, 1, 256, 256, 4, None, 1 << 30, fake, None) == -1
    assert L.dvq_rq_backward_f32(fake, fake, 1, 8, 8, 2, 1, 256, 256, 4, fake, 1 << 30, fake, None) == -1
    assert L.dvq_rq_backward_f32(fake, fake, 1, 8, 8, 1, 1, 256, 256, 4, fake, 16, fake, None) == -3
    books = (vp * 2)(fake, fake)
    ks = (ctypes.c_int * 2)(65, 65)
    emb = lambda **kw: L.dvq_rq_embed_code_f32(kw.get("books", books), ks, kw.get("depth", 2), fake, 1, 8, 8, 1, 1, 256, 256,
                                               kw.get("mode", 0), kw.get("j", 1), fake, None)
    assert emb(books=None) == -1 and emb(mode=3) == -1 and emb(j=2) == -1 and emb(depth=0) == -1
    assert emb(books=(vp * 2)(fake, None)) == -1
    assert "depth" in L.dvq_last_error_string().decode() or "codebook" in L.dvq_last_error_string().decode()


# ---- GPU --------------------------------------------------------------------------------------------------------------------

def _t(dev):
    return lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [_lib.MODE_FILTER, _lib.MODE_EXACT])
@pytest.mark.parametrize("tag", EVAL_CASES)
def test_eval_golden(dev, tag, mode):
    rec = _load(tag)
    emb = dict(np.load(os.path.join(GOLDEN, "rq_%s_embed.npz" % tag)))
    rq = _module(rec, dev).eval()
    rq.assign_mode = mode
    t = _t(dev)
    x = t(rec["x"])
    with torch.no_grad():
        out, loss, codes = rq(x)
        assert torch.equal(rq.get_codes(x), codes)
    assert np.array_equal(codes.cpu().numpy(), rec["codes"])
    assert same_bits(out.cpu().numpy(), rec["out"])
    assert loss.dim() == 0 and abs(float(loss) - float(rec["loss"])) <= 1e-5 * abs(float(rec["loss"]))
    d = int(rec["code_shape"][2])
    assert same_bits(rq.embed_code(codes).cpu().numpy(), emb["embed_code"])
    assert same_bits(rq.embed_code(codes).cpu().numpy(), rec["agg"])
    assert same_bits(rq.embed_partial_code(codes, d - 1, "add").cpu().numpy(), emb["embed_code"])
    assert same_bits(rq.embed_partial_code(codes, 1, "add").cpu().numpy(), emb["partial_add_1"])
    assert same_bits(rq.embed_partial_code(codes, 1, "select").cpu().numpy(), emb["partial_select_1"])
    ed, none = rq.embed_code_with_depth(codes, to_latent_shape=True)
    assert none is None and same_bits(ed.cpu().numpy(), emb["embed_code_with_depth"])
    ec, _ = rq.embed_code_with_depth(codes)
    books = _books(rec, d)
    assert same_bits(ec.cpu().numpy(), np.stack([books[i][rec["codes"][..., i]] for i in range(d)], -2))
    with pytest.raises(NotImplementedError):
        rq.embed_partial_code(codes, 1, "mul")


def _randperm_reversed(n, *a, **kw):
    return torch.arange(n - 1, -1, -1, device=kw.get("device"))


@pytest.mark.gpu
@pytest.mark.parametrize("tag", TRAIN_CASES)
def test_train_golden(dev, oracle_mod, tag, monkeypatch):
    rec = _load(tag)
    rq = _module(rec, dev).train()
    t = _t(dev)
    x = t(rec["x"]).requires_grad_(True)
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
    shared = bool(rec["shared"])
    for i, cb in enumerate(rq.codebooks[:1] if shared else rq.codebooks):
        for name in ("weight", "cluster_size_ema", "embed_ema"):
            got, ref = getattr(cb, name).detach().cpu().numpy(), rec["after.%s.%d" % (name, i)]
            assert np.abs(got - ref).max() <= 1e-5 * max(1.0, np.abs(ref).max()), (name, i)
    # the next eval forward searches the updated codebooks: the restatement on OUR updated weights
    rq.eval()
    with torch.no_grad():
        _, _, codes2 = rq(x.detach())
    d = int(rec["code_shape"][2])
    books = [cb.weight.detach().cpu().numpy()[:-1] for cb in ([rq.codebooks[0]] * d if shared else rq.codebooks)]
    rH, rW = int(rq.shape_divisor[0]), int(rq.shape_divisor[1])
    ref_codes, _, _, _ = _restate(oracle_mod, rec["x"], books, rH, rW)
    assert np.array_equal(codes2.cpu().numpy(), ref_codes)


def _scale_module(latent, code, n_embed, shared, dev):
    rq = RQBottleneck(latent, code, n_embed, shared_codebook=shared)
    D = rq.codebooks[0].weight.shape[1]
    books = []
    with torch.no_grad():
        for i, cb in enumerate(rq.codebooks[:1] if shared else rq.codebooks):
            E = synth.codebook_trained(cb.n_embed, D, seed=2101 + i)
            cb.weight[:-1].copy_(torch.from_numpy(E))
            books.append(E)
    return rq.to(dev).eval(), books * code[-1] if shared else books


@pytest.mark.gpu
@pytest.mark.parametrize("shared", [True, False])
def test_reference_shape_against_restatement(dev, oracle_mod, shared):
    """RQ-VAE's own setting (shared K = 16384, D = 256, depth 4, 8 x 8 grid) at B = 16, and separate codebooks at divisor 2"""
    if shared:
        rq, books = _scale_module((8, 8, 256), (8, 8, 4), 16384, True, dev)
        B, rH, rW = 16, 1, 1
    else:
        rq, books = _scale_module((8, 8, 64), (4, 4, 4), [512, 1024, 2048, 4096], False, dev)
        B, rH, rW = 16, 2, 2
    h, w = 8 // rH, 8 // rW
    z = synth.z_tokens(books[0], B, h, w, 2201)
    x = _to_latent(np.ascontiguousarray(z.transpose(0, 2, 3, 1)), rH, rW, rq.latent_shape[2])
    codes_ref, out_ref, agg_ref, loss_ref = _restate(oracle_mod, x, books, rH, rW)
    t = _t(dev)
    with torch.no_grad():
        out, loss, codes = rq(t(x))
        assert np.array_equal(codes.cpu().numpy(), codes_ref)
        assert same_bits(out.cpu().numpy(), out_ref)
        assert abs(float(loss) - loss_ref) <= 1e-5 * abs(loss_ref)
        assert same_bits(rq.embed_code(codes).cpu().numpy(), agg_ref)
        # a 4-byte-aligned (not 16-byte-aligned) x takes the scalar step kernel: the same bits
        buf = torch.empty(x.size + 1, device=dev)
        xm = buf[1:].view(x.shape)
        xm.copy_(t(x))
        outm, lossm, codesm = rq(xm)
        assert torch.equal(codesm, codes) and torch.equal(outm, out) and torch.equal(lossm, loss)
    if not shared:                                 # (the reference stacks the soft codes: codebooks of one size only)
        return
    with torch.no_grad():
        soft, hard = rq.get_soft_codes(t(x))
    assert torch.equal(hard, codes)
    assert soft.shape == (B, h, w, 4, 16384)
    assert torch.allclose(soft.sum(-1), torch.ones((), device=dev), atol=1e-4)
    _, sc = rq.get_soft_codes(t(x[:2]), temp=0.05, stochastic=True)
    assert sc.shape == (2, h, w, 4) and int(sc.min()) >= 0 and int(sc.max()) < 16384


@pytest.mark.gpu
def test_bitwise_reproducible_loss_and_grad(dev):
    rq, books = _scale_module((8, 8, 64), (4, 4, 4), [256, 256, 512, 1024], False, dev)
    z = synth.z_tokens(books[0], 16, 4, 4, 2301)
    x0 = torch.from_numpy(_to_latent(np.ascontiguousarray(z.transpose(0, 2, 3, 1)), 2, 2, 64)).to(dev)
    R = torch.from_numpy(synth.normal(2302, tuple(x0.shape))).to(dev)
    res = []
    for _ in range(2):
        x = x0.clone().requires_grad_(True)
        out, loss, codes = rq(x)
        ((out * R).sum() + 3.0 * loss).backward()
        res.append((loss.detach().clone(), x.grad.clone(), codes))
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])
    # d loss / d x alone: 2 / (numel d) sum_i (x - agg_{i+1}), summed over depth from embed_partial_code('add', i)
    x = x0.clone().requires_grad_(True)
    _, loss, codes = rq(x)
    loss.backward()
    with torch.no_grad():
        s = sum(x0 - rq.embed_partial_code(codes, i, "add") for i in range(4))
    assert torch.allclose(x.grad, s * (2.0 / (x0.numel() * 4)), rtol=1e-5, atol=1e-12)


@pytest.mark.gpu
def test_eval_forward_is_graph_capturable(dev):
    rq, books = _scale_module((8, 8, 256), (8, 8, 4), 1024, True, dev)
    mk = lambda seed: torch.from_numpy(np.ascontiguousarray(synth.z_tokens(books[0], 4, 8, 8, seed).transpose(0, 2, 3, 1))).to(dev)
    x = mk(2401)
    step = lambda: rq(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.no_grad(), torch.cuda.stream(s):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        res = step()
    x.copy_(mk(2402))
    g.replay()
    torch.cuda.synchronize()
    got = [r.clone() for r in res]
    with torch.no_grad():
        ref = step()
    for a, b in zip(got, ref):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_unserved_shapes_raise(dev):
    for latent, code in (((8, 8, 48), (8, 8, 2)), ((8, 8, 128), (4, 4, 2))):     # D = 48; D = 512
        rq = RQBottleneck(latent, code, 64).to(dev).eval()
        with pytest.raises(_lib.DvqError):
            rq(torch.zeros((1,) + latent, device=dev))
    deep = RQBottleneck((8, 8, 64), (8, 8, _lib.RQ_MAX_DEPTH + 1), 64, shared_codebook=True).to(dev).eval()
    with pytest.raises(_lib.DvqError):
        deep(torch.zeros(1, 8, 8, 64, device=dev))
    with pytest.raises(_lib.DvqError):
        deep.embed_code(torch.zeros((1, 8, 8, _lib.RQ_MAX_DEPTH + 1), dtype=torch.int64, device=dev))
