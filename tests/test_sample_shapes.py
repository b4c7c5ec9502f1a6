"""The stage-2 sampling head and the coarse -> fine position transfer (csrc/sample.hip) off the sizes of the recorded
goldens: vocabularies on and next to 256 and 8192, every coarse grid form up to 32 x 32, ties, neighbouring floats, and the
host wrapper's strides.

The head is checked stage by stage, each stage against the strongest statement that holds for it:
  mask, top-k   bit-equal to the float32 restatement (tests/_sample_ref.py): an IEEE division and an exact selection
  softmax       against float64 (R.softmax64), |p - p64| <= 1e-6 and <= 64 * 2^-24 * p64 + 1e-30.  The relative bound: expf
                is good to 2 ulp, a term of the sum passes at most 41 additions (32 strided, 6 shuffle steps, 3 wave adds),
                the division adds one rounding; 64 leaves a margin over these 46
  top-p         the kept set is exact GIVEN the kernel's own float32 softmax (R.top_p_exact with float64 masses) on every row
                whose nearest decision is further than (V + 2) * 2^-48 from top_p, the truncation of the kernel's fixed-point
                masses; at most 1 row in 100 may lie inside that margin
  draw          argmax(p / q) in float32 on the kernel's own probabilities, first index on ties
Measured on an MI355X: the softmax error reaches 0.098 of its relative bound (V = 8192), the top-p renormalisation 0.084 of
its bound, and 12 of 5257 top-p rows lie inside the margin (tied maxima whose masses land exactly on top_p, and rows at top_p = 1.0 whose float32
probabilities sum to 1 within the margin).
"""
import numpy as np
import pytest
import torch

from dynamicvectorquantization_amd import _lib
from dynamicvectorquantization_amd.sample import (SamplingRules, sample_step,
                                                  transfer_sampled_coarse_position_to_remain_fine_position,
                                                  transfer_sampled_coarse_position_to_sampled_fine_position)
from tests import _sample_ref as R

KINDS = ("coarse_position", "fine_position", "content")
VARIANTS = ("class", "class2_entropy", "uncond")
LAYOUTS = ("top", "spread")
TEMPS = (1.0, 0.7, 1.3)
VS = (2, 63, 64, 65, 255, 256, 257, 1000, 4097, 8191, 8192)
BS = (1, 3, 37)
KS = (1, 2, 17, 256)                                     # and V - 1, V
TOP_PS = (0.05, 0.3, 0.8, 0.95, 0.999, 1.0)
REL = 64 * 2.0 ** -24
NEG = R.NEG
FAMILIES = ("gauss", "ints", "zeros", "ulps", "huge", "negative")


def _rules(c, variant, order="region-first", sos=True):
    a = {k: v for k, v in R.model_attrs(c, variant, order).items() if k not in ("hw2", "activate_segment")}
    a["activate_sos_for_fine_sequence"] = sos
    return SamplingRules(variant, **a)


def _cases():
    """every (V, B) once; kind, variant, layout and temperature rotate against each other, so that over the table every kind
    meets every variant, layout and temperature, and every V every kind (test_case_table_covers_the_forms)"""
    out = []
    for i, (V, B) in enumerate([(V, B) for V in VS for B in BS] + [(65, 300)]):
        v, b = i // 3, i % 3                              # index of V and of B
        out.append(dict(V=V, B=B, kind=KINDS[(b + v) % 3], variant=VARIANTS[v % 3], layout=LAYOUTS[i % 2],
                        temp=TEMPS[(2 * b + v) % 3], seed=1000 + i, shift=i))
    return out


CASES = _cases()


def _row(g, family, V, r):
    if family == "gauss":
        return g.standard_normal(V) * 3
    if family == "ints":                                 # heavy ties at every threshold
        return g.integers(-3, 4, V).astype(np.float64)
    if family == "zeros":                                # +-0, denormals and the smallest normal
        pool = np.array([0.0, -0.0, 1e-40, -1e-40, 1.4e-45, -1.4e-45, 1.1754942e-38, 1.17549435e-38], np.float32)
        row = g.choice(pool, V)
        row[g.integers(0, V)] = 0.5                      # one larger entry: the tied probabilities are no simple fractions
        return row
    if family == "ulps":                                 # V consecutive floats, shuffled: the k-th and (k+1)-th largest are
        step = g.permutation(V)                          # nextafter neighbours for every k (some rows: in tied groups of 4)
        if (r // 6) % 2:
            step = step // 4
        return (np.float32(1.0) + step.astype(np.float32) * np.float32(2.0 ** -23)) * np.float32(-1.0 if (r // 12) % 2 else 1.0)
    if family == "huge":
        row = g.standard_normal(V)
        n = max(1, V // 16)
        big = g.choice(np.array([1e30, -1e30]), n)
        if (big > 0).sum() % 5 == 0:                     # m tied maxima have p = 1 / m: keep 4 / 5 = top_p out of the random rows
            big[0] = -big[0]
        row[g.choice(V, n, replace=False)] = big
        return row
    return -np.abs(g.standard_normal(V)) * 3 - 1


def _data(case):
    """the inputs of one case on the CPU: logits, history (position kinds), flags, q; fixed by the case's seed"""
    g = np.random.default_rng(case["seed"])
    V, B, kind, shift = case["V"], case["B"], case["kind"], case["shift"]
    c = R.codes_for(V, 4, case["layout"])
    eos = c[kind + "_eos_code"]
    logits = np.stack([np.asarray(_row(g, FAMILIES[(r + shift) % 6], V, r), np.float32) for r in range(B)])
    flag = np.array([[float(1 + r % 2) if (r + shift) % 5 == 4 else 0.0] for r in range(B)], np.float32)
    hist = None
    if kind != "content":
        for r in range(B):
            if r % 7 == 1:
                logits[r, eos] = 15.0                    # a row that mostly ends its sequence: the flag is raised
        L = 1 + min(V, 30)
        hist = g.integers(0, V, (B, L))
        hist[:, 0] = c[kind + "_sos_code"]
        if L > 4:
            hist[:, 3], hist[:, 4] = -1, V
    q = np.maximum(g.exponential(1.0, (B, V)), 1e-10).astype(np.float32)
    t = torch.from_numpy
    return dict(case, c=c, rules=_rules(c, case["variant"]), logits=t(logits), flag=t(flag), q=t(q),
                hist=None if hist is None else t(hist.astype(np.int64)),
                scaled=t(logits / np.float32(case["temp"])))


def _want_logits(d, k=None):
    x = R.mask(d["scaled"], d["kind"], d["variant"], d["c"], d["hist"], d["flag"])
    return x if k is None else R.top_k(x, k)


def _step(dev, d, top_k=None, top_p=None, sample=False):
    """one sample_step on the device with both taps; returns CPU tensors (token [B], out_logits, out_probs, flag after)"""
    B, V = d["logits"].shape
    ol, op = torch.empty((B, V), device=dev), torch.empty((B, V), device=dev)
    flag = d["flag"].to(dev)
    ix = sample_step(d["logits"].to(dev), d["kind"], d["rules"], history=None if d["hist"] is None else d["hist"].to(dev),
                     flag=flag, temperature=d["temp"], top_k=top_k, top_p=top_p, sample=sample,
                     q=d["q"].to(dev) if sample else None, out_logits=ol, out_probs=op)
    return ix.cpu()[:, 0], ol.cpu(), op.cpu(), flag.cpu()


def _bits(t):
    return t.contiguous().view(torch.int32)


def _ks(V):
    return sorted({k for k in KS + (V - 1, V) if 1 <= k <= V})


# ------------------------------------------------------------------------------------------------------------- CPU


def test_case_table_covers_the_forms():
    assert {(c["V"], c["B"]) for c in CASES} == {(V, B) for V in VS for B in BS} | {(65, 300)}
    assert {(c["kind"], c["variant"]) for c in CASES} == {(k, v) for k in KINDS for v in VARIANTS}
    assert {(c["kind"], c["layout"]) for c in CASES} == {(k, l) for k in KINDS for l in LAYOUTS}
    assert {(c["kind"], c["temp"]) for c in CASES} == {(k, t) for k in KINDS for t in TEMPS}
    for V in VS:
        assert {c["kind"] for c in CASES if c["V"] == V} == set(KINDS)
    mixed = [c for c in CASES if c["B"] >= 3 and 0 < _data(c)["flag"].bool().sum() < c["B"]]
    assert len(mixed) >= 12                               # flagged and unflagged rows in one batch


def test_codes_for_passes_the_rules_and_the_abi():
    """every dict builds SamplingRules for every variant, and dvq_sample_head_f32 accepts its rule codes: the call is stopped
    by the check that FOLLOWS the rule checks (a row stride below V), so nothing is launched"""
    import ctypes
    fake = 256                                           # never dereferenced: validation returns first
    for V in VS + (3, 4, 33, 34):
        for layout in LAYOUTS:
            c = R.codes_for(V, 4, layout)
            for kind in KINDS:
                pad, eos, sos = (c["%s_%s_code" % (kind, n)] for n in ("pad", "eos", "sos"))
                assert 0 <= pad < V and 0 <= sos < V and 0 <= eos <= V and 0 < c["max_coarse_postion_idx"] <= V
                if V >= 4:
                    assert len({pad, eos, sos}) == 3
            for variant in VARIANTS:
                r = _rules(c, variant)
                for kind in KINDS:
                    rc = _lib.lib.dvq_sample_head_f32(fake, V - 1, 2, V, 1.0, (ctypes.c_int64 * 7)(*r.codes[kind]), 0, 1, 0,
                                                      fake, 0, 0.0, 0, 0, fake, 1, 0, 0, 0)
                    msg = _lib.lib.dvq_last_error_string().decode()
                    assert rc == -1 and "bad stride" in msg, (V, layout, variant, kind, msg)
                    # an unflagged row without history keeps a finite entry
                    x = R.mask(torch.zeros(1, V), kind, variant, c, None, torch.zeros(1, 1))
                    assert torch.isfinite(x).any(), (V, layout, variant, kind)
    for hw1 in (1, 3, 17, 32):                            # the transfer's vocabulary: no code collides with a position
        c = R.codes_for(4 * hw1 * hw1 + 3, hw1, "top")
        assert min(c["coarse_position_pad_code"], c["fine_position_pad_code"]) >= 4 * hw1 * hw1 and c["fine_hw"] == 2 * hw1
    with pytest.raises(ValueError):
        R.codes_for(1, 4)


def test_float64_helpers_reproduce_the_head_goldens(golden_dir):
    import glob
    import os
    files = sorted(glob.glob(os.path.join(golden_dir, "sample_head_*.npz")))
    assert len(files) == 6
    for f in files:
        z = np.load(f)
        for kind in KINDS:
            g = lambda n: z[kind + "/" + n]
            p64 = R.softmax64(torch.from_numpy(g("masked")))
            assert p64.dtype == torch.float64 and np.abs(p64.numpy() - g("probs")).max() <= 1e-6, (f, kind)
            assert ((p64.sum(-1) - 1).abs() <= 1e-12).all()
            probs = torch.from_numpy(g("probs"))
            for p in g("ps"):
                keep, ren, margin = R.top_p_exact(probs, float(p))
                want = g("topp_%g" % p)
                assert np.array_equal((keep & (probs > 0)).numpy(), want > 0), (f, kind, p)
                assert np.abs(ren.numpy() - want).max() <= 1e-6, (f, kind, p)
                assert margin.shape == (probs.shape[0],) and margin.dtype == torch.float64


def test_top_p_exact_on_known_rows():
    p = torch.tensor([[0.25, 0.25, 0.0, 0.25, 0.25], [0.1, 0.6, 0.3, 0.0, 0.0]], dtype=torch.float32)
    keep, ren, margin = R.top_p_exact(p, 0.5)
    assert keep.tolist() == [[True, True, False, False, False], [False, True, False, False, False]]
    assert ren[0].tolist() == [0.5, 0.5, 0, 0, 0] and ren[1].tolist() == [0, 1, 0, 0, 0]
    assert margin[0].item() == 0.0 and abs(margin[1].item() - 0.1) < 1e-7      # a mass equal to top_p is not "< top_p"
    keep, _, _ = R.top_p_exact(p, 1e-9)
    assert keep.tolist() == [[True, False, False, False, False], [False, True, False, False, False]]


def test_transfer_restatement_serves_a_row_of_the_sos_alone():
    c = R.codes_for(4 * 9 + 3, 3, "top")
    cp = torch.full((2, 1), c["coarse_position_sos_code"], dtype=torch.long)
    assert not R.transfer_selected(c, cp, False).any() and R.transfer_selected(c, cp, True).all()
    assert R.transfer(c, cp, False, "row-first", None).tolist() == [[c["fine_position_eos_code"]]] * 2
    assert R.transfer(c, cp, True, "row-first", "copy")[0].tolist() == [c["coarse_position_sos_code"]] + list(range(36)) + \
        [c["fine_position_eos_code"]]


# ------------------------------------------------------------------------------------------------- GPU: the head


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
def test_mask_and_top_k_are_exact(dev, V):
    ties = neighbours = above_finite = 0
    for case in (c for c in CASES if c["V"] == V):
        d = _data(case)
        for k in [None] + _ks(V):
            _, ol, _, _ = _step(dev, d, top_k=k)
            want = _want_logits(d, k)
            assert torch.equal(ol, want), (case, k)
            assert torch.equal(_bits(ol), _bits(want)), (case, k)          # -0.0 stays -0.0
            if k is None:
                continue
            masked = _want_logits(d)
            finite = torch.isfinite(masked).sum(-1)
            kept = torch.isfinite(want).sum(-1)
            assert (kept >= torch.minimum(finite, torch.tensor(k))).all()
            ties += int((kept > k).sum())
            short = finite < k                                             # the threshold is -inf: nothing changes
            above_finite += int(short.sum())
            assert torch.equal(want[short], masked[short])
            if k < V:
                s = torch.sort(masked, -1, descending=True).values
                a, b = s[:, k - 1], s[:, k]
                neighbours += int(((a != b) & (torch.nextafter(b, torch.full_like(b, float("inf"))) == a)).sum())
    assert above_finite > 0
    if V >= 63:
        assert ties > 0 and neighbours > 0


@pytest.mark.gpu
@pytest.mark.parametrize("V", VS)
def test_softmax_against_float64(dev, V):
    worst = 0.0
    for case in (c for c in CASES if c["V"] == V):
        d = _data(case)
        for k in (None, min(17, V)):
            _, ol, op, _ = _step(dev, d, top_k=k)
            want = _want_logits(d, k)
            assert torch.equal(ol, want), (case, k)
            p64 = R.softmax64(want)
            err = (op.double() - p64).abs()
            ratio = (err / (REL * p64 + 1e-30)).max().item()
            worst = max(worst, ratio)
            print("softmax V=%d B=%d k=%s: max abs err %.3e, max err / relative bound %.4f" % (V, case["B"], k, err.max().item(),
                                                                                               ratio))
            assert err.max().item() <= 1e-6, (case, k)
            assert ratio <= 1.0, (case, k)
            assert (op[want == NEG] == 0).all() and (op <= 1).all() and (op >= 0).all()
    print("softmax V=%d: worst err / bound %.4f" % (V, worst))


def _check_top_p(p32, op, top_p, V, tag):
    """-> (rows checked, rows skipped, worst renormalisation error / bound)"""
    keep, ren, margin = R.top_p_exact(p32, top_p)
    ok = margin > (V + 2) * 2.0 ** -48
    assert torch.equal((op > 0)[ok], (keep & (p32 > 0))[ok]), tag
    err = (op.double() - ren).abs()[ok]
    bound = (REL * ren)[ok]
    assert (err <= bound).all(), tag
    worst = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    return int(ok.numel()), int((~ok).sum()), worst


@pytest.mark.gpu
def test_top_p_kept_set_given_the_kernels_softmax(dev):
    rows = skipped = 0
    worst = 0.0
    for case in CASES:
        d = _data(case)
        V = case["V"]
        for k in (None, min(17, V)):                      # k = 17 with top_p = 0.8: the chain
            _, _, p32, _ = _step(dev, d, top_k=k)
            _, _, again, _ = _step(dev, d, top_k=k)
            assert torch.equal(_bits(p32), _bits(again)), case                 # fixed order: bit-reproducible
            for top_p in (TOP_PS if k is None else (0.8,)):
                _, ol, op, _ = _step(dev, d, top_k=k, top_p=top_p)
                assert torch.equal(ol, _want_logits(d, k)), (case, k, top_p)
                n, s, w = _check_top_p(p32, op, top_p, V, (case, k, top_p))
                rows, skipped, worst = rows + n, skipped + s, max(worst, w)
    print("top-p: %d rows, %d skipped inside the fixed-point margin, worst renormalisation err / bound %.4f" %
          (rows, skipped, worst))
    assert skipped * 100 <= rows


@pytest.mark.gpu
def test_top_p_crafted_rows(dev):
    """rows whose kept set is known exactly: nothing is skipped"""
    V = 8192
    c = R.codes_for(V, 4, "top")
    rules = _rules(c, "class")
    eos = c["fine_position_eos_code"]
    g = np.random.default_rng(77)
    free = np.setdiff1d(np.arange(V), [c["fine_position_pad_code"], eos, c["fine_position_sos_code"]])
    tiny = float(np.float32(2.0 ** -12 * (1 + 2.0 ** -20)))
    for n in (4, 256, 4096):
        # n equal logits at scattered indices (the eos among them), everything else banned through the history: p = 1 / n
        # exactly, so the key's probability bits are all equal and the index bits decide every digit of the descent
        tied = np.sort(np.concatenate([g.choice(free, n - 1, replace=False), [eos]]))
        banned = np.setdiff1d(free, tied)
        logits = torch.from_numpy(g.standard_normal((2, V)).astype(np.float32))
        logits[:, tied] = 1.25
        hist = torch.from_numpy(np.stack([banned, banned[::-1]]).astype(np.int64))
        d = dict(kind="fine_position", variant="class", c=c, rules=rules, temp=1.0, logits=logits, scaled=logits.clone(),
                 hist=hist, flag=torch.zeros(2, 1), q=None)
        _, ol, p32, _ = _step(dev, d)
        assert torch.equal(ol, _want_logits(d)) and int(torch.isfinite(ol[0]).sum()) == n
        assert (p32[:, tied] == 1.0 / n).all() and p32.sum().item() == 2.0
        for top_p, count in ((0.5, n // 2), (0.25, n // 4), (1.0, n), (tiny, 2 if n == 4096 else 1), (1e-9, 1)):
            _, _, op, _ = _step(dev, d, top_p=top_p)
            want = torch.zeros(2, V)
            want[:, tied[:count]] = 1.0 / count
            assert torch.equal(op, want), (n, top_p)
            keep, ren, margin = R.top_p_exact(p32, top_p)
            assert torch.equal(keep & (p32 > 0), want > 0) and torch.equal(ren.float(), want), (n, top_p)
            if top_p == tiny:
                assert (margin > (V + 2) * 2.0 ** -48).all()
    # a tiny top_p keeps the first index of the maximum alone: a one-hot row, whatever the row holds
    for case in (CASES[10], CASES[17], CASES[30], CASES[32]):
        d = _data(case)
        _, _, p32, _ = _step(dev, d)
        _, _, op, _ = _step(dev, d, top_p=1e-9)
        want = torch.zeros_like(p32)
        want[torch.arange(p32.shape[0]), torch.from_numpy(np.argmax(p32.numpy(), -1))] = 1.0
        assert torch.equal(op, want), case


@pytest.mark.gpu
def test_draw_flag_and_write_back(dev):
    raised = 0
    for case in CASES:
        d = _data(case)
        V, kind = case["V"], case["kind"]
        for k, top_p in ((None, None), (min(17, V), 0.8)):
            for sample in (True, False):
                tok, _, op, flag = _step(dev, d, top_k=k, top_p=top_p, sample=sample)
                score = op.numpy() / d["q"].numpy() if sample else op.numpy()
                assert score.dtype == np.float32
                assert np.array_equal(tok.numpy(), np.argmax(score, -1)), (case, k, top_p, sample)   # first index on ties
                hit = (tok == d["c"][kind + "_eos_code"]).float()[:, None] if kind != "content" else 0.0
                assert torch.equal(flag, d["flag"] + hit), (case, k, top_p, sample)
                raised += int(torch.as_tensor(hit).sum())
                flagged = d["flag"][:, 0] != 0
                assert (tok[flagged] == d["c"][kind + "_pad_code"]).all()
    assert raised > 0
    # the top two probabilities equal: greedy takes the first index, the draw follows q
    V = 257
    c = R.codes_for(V, 4, "top")
    logits = torch.from_numpy(np.random.default_rng(5).standard_normal((3, V)).astype(np.float32))
    logits[:, 200] = logits[:, 13] = 9.0
    q = torch.ones(3, V)
    q[1, 200], q[2, 13] = 0.5, 0.5
    d = dict(kind="content", variant="class", c=c, rules=_rules(c, "class"), temp=1.0, logits=logits, hist=None,
             flag=torch.zeros(3, 1), q=q)
    tok, _, op, flag = _step(dev, d)
    assert torch.equal(_bits(op[:, 13]), _bits(op[:, 200])) and (op.argmax(-1) == 13).all()
    assert tok.tolist() == [13, 13, 13] and not flag.any()
    tok, _, _, _ = _step(dev, d, sample=True)
    assert tok.tolist() == [13, 200, 13]


@pytest.mark.gpu
def test_head_addressing(dev):
    V, B = 1000, 5
    g = np.random.default_rng(31)
    c = R.codes_for(V, 4, "spread")
    rules = _rules(c, "class")
    kind = "fine_position"
    flag = torch.zeros(B, 1)
    # logits [B, T, V]: the last step is read in place through the row stride
    logits3 = torch.from_numpy(g.standard_normal((B, 3, V)).astype(np.float32) * 3).to(dev)
    last = logits3[:, -1, :].cpu()
    # a history that is a column slice of a wider buffer, shorter than the slice: the columns past history_len are not banned
    wide = torch.from_numpy(g.permutation(V)[:B * 60].reshape(B, 60).astype(np.int64)).to(dev)
    view = wide[:, 3:40]
    ol = torch.empty(B, V, device=dev)
    sample_step(logits3, kind, rules, history=view, history_len=20, flag=flag.to(dev), sample=False, out_logits=ol)
    want = R.mask(last, kind, "class", c, view[:, :20].cpu(), flag)
    assert torch.equal(ol.cpu(), want)
    assert not torch.equal(want, R.mask(last, kind, "class", c, view.cpu(), flag))
    assert not torch.equal(want, R.mask(logits3[:, 0, :].cpu(), kind, "class", c, view[:, :20].cpu(), flag))
    # 700 entries: three passes of the 256 threads; duplicates, -1, V and 2^40 among them
    long_ = g.integers(0, V, (B, 700))
    long_[:, 600:] = long_[:, :100]
    long_[:, 5], long_[:, 300], long_[:, 699], long_[:, 511] = -1, V, 2 ** 40, -2 ** 40
    buf = torch.zeros(B, 900, dtype=torch.long)
    buf[:, 100:800] = torch.from_numpy(long_)
    hist = buf.to(dev)[:, 100:800]
    sample_step(logits3, kind, rules, history=hist, flag=flag.to(dev), sample=False, out_logits=ol)
    want = R.mask(last, kind, "class", c, hist.cpu(), flag)
    assert torch.equal(ol.cpu(), want) and int((want == NEG).sum()) > B * 400
    # out / column: the token lands in the middle column, the others stay
    q = torch.from_numpy(g.exponential(1.0, (B, V)).astype(np.float32)).to(dev)
    plain = sample_step(logits3, kind, rules, history=hist, flag=flag.to(dev), top_k=50, top_p=0.9, q=q)
    seq = torch.full((B, 5), -7, dtype=torch.long, device=dev)
    ix = sample_step(logits3, kind, rules, history=hist, flag=flag.to(dev), top_k=50, top_p=0.9, q=q, out=seq, column=2)
    assert ix.data_ptr() == seq[:, 2:3].data_ptr() and torch.equal(ix, plain)
    assert torch.equal(seq[:, 2:3], plain) and (seq[:, [0, 1, 3, 4]] == -7).all()


# -------------------------------------------------------------------------------------------- GPU: the transfer

GRIDS = (1, 2, 3, 5, 8, 15, 16, 17, 20, 31, 32)
SOS = (("class", True, "const"), ("class2_entropy", True, "copy"), ("uncond", False, None))
ORDERS = ("region-first", "row-first")


def _transfer_rows(hw1, c, g):
    """coarse position rows [B, hw1^2 + 40] for one grid: column 0 the sos (a label of the row), then the sampled cells"""
    n = hw1 * hw1
    Lc = n + 40
    pad, eos = c["coarse_position_pad_code"], c["coarse_position_eos_code"]
    rows = []

    def row(entries):
        r = np.full(Lc, pad, np.int64)
        r[0] = 100 + len(rows)
        e = np.asarray(entries, np.int64)[:Lc - 1]
        r[1:1 + len(e)] = e
        rows.append(r)

    cells = lambda frac: np.flatnonzero(g.random(n) < frac)
    row(g.integers(0, n, Lc - 1))                                           # no EOS
    row([eos] + list(g.integers(0, n, 5)))                                  # EOS in column 1: nothing sampled
    row(list(g.permutation(n)) + [eos])                                     # every cell
    row([n - 1, eos])                                                       # one cell
    # a full grid row next to an empty one, at the grid row that holds cell 255 (where a chunk of 256 cells ends), both ways
    full = min(255 // hw1, hw1 - 1)
    other = full + 1 if full + 1 < hw1 else max(full - 1, 0)
    for a, b in ((full, other), (other, full)):
        m = g.random((hw1, hw1)) < 0.5
        m[b] = False
        m[a] = True
        row(list(g.permutation(np.flatnonzero(m.reshape(-1)))) + [eos])
    dup = g.integers(0, n, max(n // 2, 2))
    row(list(dup) + list(dup[::-1]) + [eos])                                # duplicates
    row([n - 1, pad, -1, -5, n, n + 3, 2 ** 40, 0, pad, eos])               # pad / negative / >= hw1^2 before the EOS
    some = g.permutation(n)
    row(list(some[:n // 3]) + [eos] + list(some[n // 3:2 * n // 3]) + [eos] + list(some[2 * n // 3:]))   # a second EOS
    row(list(cells(0.1)) + [eos])
    row(list(g.permutation(cells(0.9))) + [eos])
    row(list(range(n - hw1, n)) + [eos])                                    # the last grid row alone
    return torch.from_numpy(np.stack(rows))


def _transfer_fn(remain):
    return transfer_sampled_coarse_position_to_remain_fine_position if remain else \
        transfer_sampled_coarse_position_to_sampled_fine_position


@pytest.mark.gpu
@pytest.mark.parametrize("hw1", GRIDS)
def test_transfer_at_every_grid_form(dev, hw1):
    n = hw1 * hw1
    c = R.codes_for(4 * n + 3, hw1, LAYOUTS[GRIDS.index(hw1) % 2])
    cp = _transfer_rows(hw1, c, np.random.default_rng(500 + hw1))
    B, Lc = cp.shape
    assert Lc == n + 40 and B == 12
    wider = torch.full((B, Lc + 9), c["coarse_position_eos_code"], dtype=torch.long)
    wider[:, 4:4 + Lc] = cp
    forms = (("rows", cp.to(dev), cp), ("slice", wider.to(dev)[:, 4:4 + Lc], cp), ("Lc=1", cp[:, :1].to(dev), cp[:, :1]))
    for variant, sos_on, sos in SOS:
        for order in ORDERS:
            r = _rules(c, variant, order, sos_on)
            for remain in (False, True):
                fn = _transfer_fn(remain)
                for name, dev_rows, cpu_rows in forms:
                    want = R.transfer(c, cpu_rows, remain, order, sos)
                    got = fn(r, dev_rows).cpu()
                    assert torch.equal(got, want), (hw1, variant, order, remain, name)
                want = R.transfer(c, cp, remain, order, sos)
                L = want.shape[1]
                got = fn(r, cp.to(dev), max_len=L + 3).cpu()                # a pad tail
                assert torch.equal(got[:, :L], want) and (got[:, L:] == c["fine_position_pad_code"]).all()
                for short in sorted({1, 2, L // 2, L - 1} - {0, L}):        # too short: exactly the prefix
                    got = fn(r, cp.to(dev), max_len=short).cpu()
                    assert torch.equal(got, want[:, :short]), (hw1, variant, order, remain, short)
    # the count kernel on its own: per-row counts and their maximum
    for remain in (False, True):
        sel = R.transfer_selected(c, cp, remain).sum(-1)
        for rows in (cp.to(dev), wider.to(dev)[:, 4:4 + Lc]):
            counts = torch.full((B,), -1, dtype=torch.int32, device=dev)
            mx = torch.full((1,), -1, dtype=torch.int32, device=dev)
            with _lib.on_device(dev):
                _lib.checked.dvq_sample_transfer_count_i64(rows.data_ptr(), rows.stride(0), B, Lc, hw1,
                                                           c["coarse_position_eos_code"], int(remain), counts.data_ptr(),
                                                           mx.data_ptr(), _lib.stream_ptr(dev))
            assert torch.equal(counts.cpu().long(), sel) and int(mx.item()) == int(sel.max())


@pytest.mark.gpu
def test_transfer_rejects_a_grid_of_33(dev):
    c = R.codes_for(4 * 33 * 33 + 3, 33, "top")
    cp = torch.zeros(2, 8, dtype=torch.long, device=dev)
    for remain in (False, True):
        with pytest.raises(_lib.DvqError):
            _transfer_fn(remain)(_rules(c, "class"), cp)
        with pytest.raises(_lib.DvqError):
            _transfer_fn(remain)(_rules(c, "class"), cp, max_len=10)
