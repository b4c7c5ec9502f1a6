"""Stage-2 sampling: the fused sampling head, the coarse -> fine position transfer, the FusedSampling loop and the permuter's
reference attributes, against golden data of the reference's own Dualformer classes (tools/gen_golden_sample.py) and the
test-side restatement in tests/_sample_ref.py."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib
from dynamicvectorquantization_amd.permuter import DualGrainSeperatePermuter
from dynamicvectorquantization_amd.sample import (FusedSampling, SamplingRules, sample_step,
                                                  transfer_sampled_coarse_position_to_remain_fine_position,
                                                  transfer_sampled_coarse_position_to_sampled_fine_position)
from tests import _sample_ref as R

KINDS = ("coarse_position", "fine_position", "content")
VKEY = {"coarse_position": "V_coarse", "fine_position": "V_fine", "content": "V_content"}


def _head_files(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "sample_head_*.npz")))
    assert len(files) == 6
    return files


def _codes(z):
    return {k[5:]: int(z[k]) for k in z.files if k.startswith("code/")}


def _rules(c, variant, order="region-first"):
    return SamplingRules(variant, **{k: v for k, v in R.model_attrs(c, variant, order).items()
                                     if k not in ("hw2", "activate_segment")})


class _StubModel(FusedSampling):
    def __init__(self, c, variant, order):
        for k, v in R.model_attrs(c, variant, order).items():
            setattr(self, k, v)
        self.sampling_variant = variant
        self.transformer = R.StubTransformer(c)


LOOP = [("class_plain", "class", "region-first", False, True, 1.0, (None, None, None, None)),
        ("class_filters", "class", "region-first", False, True, 0.7, (5, 0.9, 8, 0.95)),
        ("class_fix", "class", "row-first", True, True, 1.0, (5, 0.9, None, None)),
        ("class_greedy", "class", "row-first", False, False, 1.0, (None, None, None, None)),
        ("class2_filters", "class2_entropy", "region-first", False, True, 1.0, (7, 0.85, 6, 0.9)),
        ("class2_fix_greedy", "class2_entropy", "region-first", True, False, 1.0, (None, None, None, None)),
        ("class2_plain_rowfirst", "class2_entropy", "row-first", False, True, 1.3, (None, None, None, None)),
        ("uncond_filters", "uncond", "region-first", False, True, 1.0, (5, 0.9, 8, 0.95)),
        ("uncond_fix_greedy", "uncond", "row-first", True, False, 1.0, (None, None, None, None))]


# ------------------------------------------------------------------------------------------------------------- CPU


def test_restatement_reproduces_head_goldens(golden_dir):
    for f in _head_files(golden_dir):
        z = np.load(f)
        c, variant = _codes(z), str(z["variant"])
        for kind in KINDS:
            g = lambda n: z[kind + "/" + n]
            logits, flag, hist = torch.from_numpy(g("logits")), torch.from_numpy(g("flag")), torch.from_numpy(g("history"))
            masked = R.mask(logits, kind, variant, c, hist, flag)
            assert np.array_equal(masked.numpy(), g("masked")), (f, kind)
            for k in g("ks"):
                assert np.array_equal(R.top_k(masked, int(k)).numpy(), g("topk_%d" % k)), (f, kind, k)
            probs = torch.softmax(masked, -1)
            assert np.abs(probs.numpy() - g("probs")).max() <= 1e-6
            for p in g("ps"):
                assert np.abs(R.top_p(torch.from_numpy(g("probs")), float(p)).numpy() - g("topp_%g" % p)).max() <= 1e-6, (f, kind, p)
            chain = torch.from_numpy(g("chain_probs"))
            assert np.array_equal(torch.argmax(chain / torch.from_numpy(g("q")), -1).numpy(), g("token_sample")[:, 0])
            assert np.array_equal(torch.argmax(chain, -1).numpy(), g("token_greedy")[:, 0])


def test_restatement_reproduces_transfer_goldens(golden_dir):
    z = np.load(os.path.join(golden_dir, "sample_transfer.npz"))
    c = _codes(z)
    cp = torch.from_numpy(z["coarse_position"])
    for variant, sos in (("class", "const"), ("class2_entropy", "copy")):
        for order in ("region-first", "row-first"):
            for which in ("sampled", "remain"):
                got = R.transfer(c, cp, which == "remain", order, sos)
                assert np.array_equal(got.numpy(), z["%s/%s/%s" % (variant, order, which)]), (variant, order, which)


def test_restatement_reproduces_loop_goldens(golden_dir):
    z = np.load(os.path.join(golden_dir, "sample_loop.npz"))
    c = R.codes_small()
    for name, variant, order, fix, sample, temp, (k, p, kp, pp) in LOOP:
        g = torch.Generator().manual_seed(int(z[name + "/seed"]))
        out = R.sample_loop(R.namespace(c, variant, order), variant, c, R.conditioning(c, int(z["B"])), temp, sample, k, p, kp, pp,
                            fix, generator=g)
        for key, t in zip(("coarse", "fine", "pos_coarse", "pos_fine"), out):
            assert np.array_equal(t.numpy(), z["%s/%s" % (name, key)]), (name, key)


def test_permuter_reference_attributes(golden_dir):
    z = np.load(os.path.join(golden_dir, "sample_permuter.npz"))
    for order in ("region-first", "row-first"):
        p = DualGrainSeperatePermuter(fine_position_order=order)
        for name in ("content_eos_tensor", "coarse_position_eos_tensor", "fine_position_eos_tensor", "position_sequence_coarse",
                     "position_sequence_fine"):
            t = getattr(p, name)
            ref = z["%s/%s" % (order, name)]
            assert t.dtype == torch.int64 and tuple(t.shape) == ref.shape and np.array_equal(t.numpy(), ref), (order, name)
    assert tuple(DualGrainSeperatePermuter(fine_position_order="region-first").position_sequence_fine.shape) == (16, 16, 4)
    assert tuple(DualGrainSeperatePermuter(fine_position_order="row-first").position_sequence_fine.shape) == (32, 32)


def test_sample_abi_validation_without_gpu():
    L = _lib.lib
    fake = 256                                           # never dereferenced: validation returns first
    rules = lambda *v: (ctypes.c_int64 * 7)(*v)
    ok = rules(5, -1, 8, 7, -1, -1, 7)

    def head(logits=fake, B=2, V=16, temp=1.0, r=ok, hist=0, hlen=0, flag=fake, k=0, p=0.0, sample=0, q=0, tok=fake):
        return L.dvq_sample_head_f32(logits, V, B, V, temp, r, hist, max(hlen, 1), hlen, flag, k, p, sample, q, tok, 1, 0, 0, 0)

    assert head(logits=0) == -1
    assert head(flag=0) == -1 and head(tok=0) == -1
    assert head(sample=1, q=0) == -1                      # a draw needs q
    assert head(hlen=3, hist=0) == -1
    assert head(k=-1) == -1 and head(k=17) == -1
    assert head(p=1.5) == -1 and head(p=-0.1) == -1 and head(p=float("nan")) == -1
    assert head(temp=0.0) == -1 and head(temp=-1.0) == -1
    assert head(r=rules(16, -1, 8, 7, -1, -1, 7)) == -1   # pad outside [0, V)
    assert head(r=rules(5, -1, 8, 16, -1, -1, 7)) == -1   # restore outside [0, V)
    assert head(r=rules(5, -2, 8, 7, -1, -1, 7)) == -1
    assert head(r=rules(5, -1, 17, 7, -1, -1, 7)) == -1   # ban_from beyond V
    assert head(V=8193) == -2                             # above the vocabulary limit
    assert head(B=0) == -1
    cnt = lambda **a: L.dvq_sample_transfer_count_i64(a.get("cp", fake), 20, 2, 20, a.get("hc", 16), 257, a.get("variant", 0),
                                                      fake, fake, 0)
    assert cnt(cp=0) == -1 and cnt(variant=2) == -1 and cnt(hc=33) == -2
    fill = lambda **a: L.dvq_sample_transfer_fill_i64(fake, 20, 2, 20, 16, 257, 0, a.get("order", 0), a.get("sos", 1), 1026,
                                                      1025, 1024, a.get("L", 10), a.get("out", fake), 0)
    assert fill(out=0) == -1 and fill(order=2) == -1 and fill(sos=3) == -1 and fill(L=0) == -1
    assert _lib.lib.dvq_version() >= 900


def test_rules_reject_other_fine_ratios():
    c = dict(R.codes_small(), fine_hw=12)
    with pytest.raises(NotImplementedError):
        _rules(c, "class")


def test_sample_rejects_cpu_tensors():
    c = R.codes_small()
    r = _rules(c, "class")
    with pytest.raises(_lib.DvqError):
        sample_step(torch.zeros(2, 1, c["V_content"]), "content", r)
    with pytest.raises(_lib.DvqError):
        transfer_sampled_coarse_position_to_sampled_fine_position(r, torch.zeros(2, 5, dtype=torch.long))


# ------------------------------------------------------------------------------------------------------------- GPU


@pytest.mark.gpu
def test_multinomial_is_argmax_over_exponential_on_device(dev):
    p = torch.softmax(torch.randn(64, 1258, device=dev) * 3, -1)
    for seed in (1, 2, 3):
        g1 = torch.Generator(device=dev).manual_seed(seed)
        g2 = torch.Generator(device=dev).manual_seed(seed)
        a = torch.multinomial(p, 1, generator=g1)[:, 0]
        b = torch.argmax(p / torch.empty_like(p).exponential_(1, generator=g2), -1)
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_head_matches_goldens(dev, golden_dir):
    for f in _head_files(golden_dir):
        z = np.load(f)
        c, variant = _codes(z), str(z["variant"])
        r = _rules(c, variant)
        for kind in KINDS:
            g = lambda n: torch.from_numpy(z[kind + "/" + n]).to(dev)
            logits, hist = g("logits"), g("history")
            B, V = logits.shape
            hist_arg = hist if kind != "content" else None
            ol, op = torch.empty_like(logits), torch.empty_like(logits)
            flag = g("flag").clone()
            sample_step(logits[:, None, :], kind, r, history=hist_arg, flag=flag, sample=False, out_logits=ol, out_probs=op)
            assert torch.equal(ol, g("masked")), (f, kind)
            assert (op - g("probs")).abs().max().item() <= 1e-6, (f, kind)
            for k in z[kind + "/ks"]:
                sample_step(logits, kind, r, history=hist_arg, flag=g("flag").clone(), top_k=int(k), sample=False, out_logits=ol)
                assert torch.equal(ol, g("topk_%d" % k)), (f, kind, k)
            for p in z[kind + "/ps"]:
                sample_step(logits, kind, r, history=hist_arg, flag=g("flag").clone(), top_p=float(p), sample=False, out_probs=op)
                assert (op - g("topp_%g" % p)).abs().max().item() <= 1e-6, (f, kind, p)
            k0, p0 = int(z[kind + "/chain_k"]), float(z[kind + "/chain_p"])
            for sample, tok in ((True, "token_sample"), (False, "token_greedy")):
                flag = g("flag").clone()
                ix = sample_step(logits, kind, r, history=hist_arg, flag=flag, top_k=k0, top_p=p0, sample=sample, q=g("q"),
                                 out_probs=op)
                assert (op - g("chain_probs")).abs().max().item() <= 1e-6
                assert torch.equal(ix, g(tok)), (f, kind, tok)
                eos = r.codes[kind][6]
                want = g("flag") + ((g(tok) == eos) if eos >= 0 else 0)
                assert torch.equal(flag, want.float()), (f, kind)


@pytest.mark.gpu
def test_transfer_matches_goldens_and_restatement(dev, golden_dir):
    z = np.load(os.path.join(golden_dir, "sample_transfer.npz"))
    c = _codes(z)
    cp = torch.from_numpy(z["coarse_position"]).to(dev)
    for variant in ("class", "class2_entropy"):
        for order in ("region-first", "row-first"):
            r = _rules(c, variant, order)
            ref = z["%s/%s/sampled" % (variant, order)]
            assert np.array_equal(transfer_sampled_coarse_position_to_sampled_fine_position(r, cp).cpu().numpy(), ref)
            ref = z["%s/%s/remain" % (variant, order)]
            assert np.array_equal(transfer_sampled_coarse_position_to_remain_fine_position(r, cp).cpu().numpy(), ref)
            got = transfer_sampled_coarse_position_to_remain_fine_position(r, cp, max_len=ref.shape[1] + 3).cpu().numpy()
            assert np.array_equal(got[:, :ref.shape[1]], ref) and (got[:, ref.shape[1]:] == c["fine_position_pad_code"]).all()
    # B = 256 random sampled rows at the real sizes
    g = torch.Generator().manual_seed(5)
    B, Lc = 256, 300
    cp = torch.full((B, Lc), c["coarse_position_pad_code"], dtype=torch.long)
    cp[:, 0] = c["coarse_position_sos_code"]
    for b in range(B):
        n = int(torch.randint(0, 257, (1,), generator=g))
        cp[b, 1:1 + n] = torch.randint(0, 256, (n,), generator=g)
        if n < Lc - 1 and b % 7:
            cp[b, 1 + n] = c["coarse_position_eos_code"]
    for variant, sos in (("class", "const"), ("class2_entropy", "copy")):
        for order in ("region-first", "row-first"):
            r = _rules(c, variant, order)
            for fn, remain in ((transfer_sampled_coarse_position_to_sampled_fine_position, False),
                               (transfer_sampled_coarse_position_to_remain_fine_position, True)):
                want = R.transfer(c, cp, remain, order, sos)
                assert torch.equal(fn(r, cp.to(dev)).cpu(), want), (variant, order, remain)


@pytest.mark.gpu
def test_fused_loop_reproduces_reference_runs(dev, golden_dir):
    z = np.load(os.path.join(golden_dir, "sample_loop.npz"))
    c = R.codes_small()
    for name, variant, order, fix, sample, temp, (k, p, kp, pp) in LOOP:
        m = _StubModel(c, variant, order)
        g = torch.Generator().manual_seed(int(z[name + "/seed"]))
        out = m.sample_from_scratch(*R.conditioning(c, int(z["B"]), dev), temperature=temp, sample=sample, top_k=k, top_p=p,
                                    top_k_pos=kp, top_p_pos=pp, process=False, fix_fine_position=fix, generator=g)
        for key, t in zip(("coarse", "fine", "pos_coarse", "pos_fine"), out):
            assert np.array_equal(t.cpu().numpy(), z["%s/%s" % (name, key)]), (name, key)


@pytest.mark.gpu
def test_fused_loop_with_device_generator_equals_restated_loop(dev):
    c = R.codes_small()
    B = 16
    for variant, order, fix, filt in (("class", "region-first", False, (5, 0.9, 8, 0.95)), ("class2_entropy", "row-first", False,
                                      (None, None, None, None)), ("uncond", "region-first", True, (None, 0.9, None, None))):
        m = _StubModel(c, variant, order)
        cond = R.conditioning(c, B, dev)
        got = m.sample_from_scratch(*cond, top_k=filt[0], top_p=filt[1], top_k_pos=filt[2], top_p_pos=filt[3], process=False,
                                    fix_fine_position=fix, generator=torch.Generator(device=dev).manual_seed(3))
        want = R.sample_loop(R.namespace(c, variant, order), variant, c, cond, 1.0, True, *filt, fix,
                             generator=torch.Generator(device=dev).manual_seed(3))
        for a, b in zip(got, want):
            assert torch.equal(a, b), variant


@pytest.mark.gpu
def test_determinism_and_graph_capture(dev):
    c = R.codes_small()
    m = _StubModel(c, "class", "region-first")
    runs = [m.sample_from_scratch(*R.conditioning(c, 8, dev), top_k=5, top_p=0.9, process=False,
                                  generator=torch.Generator(device=dev).manual_seed(11)) for _ in range(2)]
    assert all(torch.equal(a, b) for a, b in zip(*runs))
    # one token-only step captured into a graph, replayed on new logits
    B, V = 32, 1258
    logits = torch.randn(B, 2, V, device=dev)
    hist = torch.randint(0, 16, (B, 5), device=dev)
    q = torch.empty(B, V, device=dev).exponential_(1)
    flag = torch.zeros(B, 1, device=dev)
    seq = torch.zeros(B, 4, dtype=torch.long, device=dev)
    rc = dict(c, max_coarse_postion_idx=255, coarse_position_pad_code=256, coarse_position_eos_code=257)
    r = _rules(rc, "class")
    kw = dict(history=hist, flag=flag, top_k=50, top_p=0.9, q=q, out=seq, column=2)
    sample_step(logits, "coarse_position", r, **kw)                                 # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        sample_step(logits, "coarse_position", r, **kw)
    for seed in range(3):
        logits.copy_(torch.randn(B, 2, V, device=dev, generator=torch.Generator(device=dev).manual_seed(seed)))
        flag.zero_()
        graph.replay()
        got = seq[:, 2].clone()
        flag.zero_()
        want = sample_step(logits, "coarse_position", r, **dict(kw, out=None))
        assert torch.equal(got, want[:, 0])
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_sample_errors(dev):
    c = R.codes_small()
    r = _rules(c, "class")
    with pytest.raises(_lib.DvqError):
        sample_step(torch.zeros(2, 1, c["V_content"], device=dev, dtype=torch.bfloat16), "content", r)
    with pytest.raises(_lib.DvqError):
        sample_step(torch.zeros(2, 1, _lib.SAMPLE_MAX_V + 1, device=dev), "content", r)
    with pytest.raises(_lib.DvqError):
        sample_step(torch.zeros(2, 1, c["V_content"]), "content", r)
    with pytest.raises(_lib.DvqError):
        sample_step(torch.zeros(2, 1, c["V_content"], device=dev), "content", r, top_k=0)


class _GradCheckingStub(R.StubTransformer):
    """a stub with a parameter, as a real transformer has: every call asserts that autograd is off"""

    def __init__(self, c):
        super().__init__(c)
        self.w = torch.nn.Parameter(torch.ones(()))

    def _tab(self, key, ref):
        assert not torch.is_grad_enabled(), "sample_from_scratch runs the transformer with autograd on"
        return super()._tab(key, ref) * self.w.to(ref.device)


def test_fused_loop_calls_the_transformer_without_autograd():
    """on CPU tensors the first transformer call runs (and asserts autograd is off), then the head refuses the CPU logits"""
    c = R.codes_small()
    m = _StubModel(c, "class", "region-first")
    m.transformer = _GradCheckingStub(c)
    with pytest.raises(_lib.DvqError):
        m.sample_from_scratch(*R.conditioning(c, 2), process=False)


@pytest.mark.gpu
def test_fused_loop_runs_without_autograd(dev):
    """like the reference's @torch.no_grad() sample_from_scratch: no graph is kept across the loop"""
    c = R.codes_small()
    m = _StubModel(c, "class", "region-first")
    m.transformer = _GradCheckingStub(c)
    assert torch.is_grad_enabled()
    out = m.sample_from_scratch(*R.conditioning(c, 4, dev), process=False, generator=torch.Generator().manual_seed(0))
    assert torch.is_grad_enabled() and all(not t.requires_grad for t in out)
