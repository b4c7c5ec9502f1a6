"""Golden data of stage-2 sampling, from the reference's own Dualformer classes (CPU; needs a checkout of the reference, imported
through oracle.refimport; the tests read only the .npz files this writes).

  sample_head_<variant>_v<V>.npz   for the three variants (class, class2_entropy, uncond) at the stub model's small vocabularies
                                   (coarse 19 / fine 67 / content 40) and at V = 2026 (every kind, real codes): per step kind
                                   the inputs (logits, mixed 0/1 flags, history), the reference helper's masked logits,
                                   top_k_logits for a few k, softmax, top_p_logits for a few p, and the tokens of the chain
                                   mask -> top_k -> softmax -> top_p: greedy, and torch.multinomial with the q its seed draws
  sample_transfer.npz              transfer_sampled_coarse_position_to_{sampled,remain}_fine_position of class (sos constant)
                                   and class2_entropy (sos copied), both orders, eos mid-row and repeated positions
  sample_permuter.npz              the reference permuter's tensor attributes, both orders
  sample_loop.npz                  whole sample_from_scratch runs of the reference classes with the stub transformer of
                                   tests/_sample_ref.py: per case the seed, the 4 returned sequences and the smallest margins
Seeds are chosen so that every draw's best p/q (or p) leads the second by a relative 1e-4 and no top-p cumulative sum lies
within 1e-5 of p: last-bit softmax differences between devices cannot flip a token.

    python tools/gen_golden_sample.py
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import refimport  # noqa: E402
from tests import _sample_ref as R  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
VARIANT_MODULES = {"class": "dqtransformer_class", "class2_entropy": "dqtransformer_class2_entropy",
                   "uncond": "dqtransformer_uncond_entropy"}
MARGIN, CUT_MARGIN = 1e-4, 1e-5


def _ref(variant):
    refimport.setup()
    import importlib
    return importlib.import_module("models.stage2_dynamic." + VARIANT_MODULES[variant])


def _permuter(order, hw1, fine_hw, c):
    refimport.setup()
    from modules.dynamic_modules.permuter import DualGrainSeperatePermuter
    return DualGrainSeperatePermuter(coarse_hw=hw1, fine_hw=fine_hw, content_pad_code=c["content_pad_code"],
                                     content_eos_code=c["content_eos_code"], coarse_position_pad_code=c["coarse_position_pad_code"],
                                     coarse_position_eos_code=c["coarse_position_eos_code"],
                                     fine_position_pad_code=c["fine_position_pad_code"],
                                     fine_position_eos_code=c["fine_position_eos_code"], fine_position_order=order)


def _model(variant, c, order, transformer=None):
    """a reference Dualformer of `variant` without its __init__ (which would build the stage-1 model): the attributes its
    __init__ sets, the permuter tensors it clones, and the given transformer"""
    cls = _ref(variant).Dualformer
    m = cls.__new__(cls)
    torch.nn.Module.__init__(m)
    for k, v in R.model_attrs(c, variant, order).items():
        setattr(m, k, v)
    p = _permuter(order, c["hw1"], c["fine_hw"], c)
    m.permuter = p
    m.fine_position_eos_tensor = p.fine_position_eos_tensor.clone()
    m.position_sequence_fine = p.position_sequence_fine.clone()
    if transformer is not None:
        m.transformer = transformer
    return m


def codes_2026():
    return dict(content_pad_code=1024, content_eos_code=1025, content_sos_code=1026, coarse_position_pad_code=256,
                coarse_position_eos_code=257, coarse_position_sos_code=258, fine_position_pad_code=1024,
                fine_position_eos_code=1025, fine_position_sos_code=1026, max_coarse_postion_idx=255, hw1=16, fine_hw=32,
                V_content=2026, V_coarse=2026, V_fine=2026)


def _ratio_margin(r):
    top = torch.topk(r, 2, dim=-1).values
    return float(((top[:, 0] - top[:, 1]) / top[:, 0]).min())


def _cut_margin(probs, p):
    cum = torch.cumsum(torch.sort(probs, dim=-1, descending=True).values, dim=-1)
    return float((cum - p).abs().min())


def gen_head(variant, c, tag, B=6):
    refimport.setup()
    from models.stage2.utils import top_k_logits, top_p_logits
    import torch.nn.functional as F
    m = _model(variant, c, "region-first")
    rec = {}
    for kind, vkey in (("coarse_position", "V_coarse"), ("fine_position", "V_fine"), ("content", "V_content")):
        V = c[vkey]
        for seed in range(1000):
            g = torch.Generator().manual_seed(seed * 7 + len(kind) + V)
            logits = torch.randn((B, V), generator=g) * 2.5
            flag = torch.tensor([[0.], [1.], [0.], [0.], [1.], [0.]])[:B]
            if kind == "coarse_position":
                n = min(40, c["hw1"] ** 2 // 2)
                hist = torch.cat([torch.full((B, 1), c["coarse_position_sos_code"]),
                                  torch.stack([torch.randperm(c["hw1"] ** 2, generator=g)[:n] for _ in range(B)])], 1)
                masked = m.avoid_repeat_or_enforce_pad_for_coarse_position(logits, hist, flag)
            elif kind == "fine_position":
                n = min(120, c["fine_hw"] ** 2 // 2)
                pos = torch.stack([torch.randperm(c["fine_hw"] ** 2, generator=g)[:n] for _ in range(B)])
                hist = torch.cat([torch.full((B, 1), c["fine_position_sos_code"]), pos,
                                  torch.full((B, 1), c["fine_position_eos_code"]), torch.full((B, 2), c["fine_position_pad_code"]),
                                  pos[:, :3]], 1)                       # eos and pad inside, repeats
                masked = m.avoid_repeat_or_enforce_pad_for_fine_position(logits, hist, flag)
            else:
                hist = torch.zeros((B, 0), dtype=torch.long)
                masked = m.avoid_special_or_enforce_pad_for_content(logits, flag)
            ks = [k for k in (1, 3, 17, 200) if k <= V]
            ps = (0.3, 0.8, 0.95)
            k0, p0 = ks[2] if len(ks) > 2 else ks[-1], 0.8
            chain = F.softmax(top_k_logits(masked, k0), dim=-1)
            if _cut_margin(chain, p0) < CUT_MARGIN:
                continue
            chain = top_p_logits(chain, p0)
            torch.manual_seed(seed)
            state = torch.get_rng_state()
            tok = torch.multinomial(chain, 1)
            torch.set_rng_state(state)
            q = torch.empty_like(chain).exponential_(1)
            assert torch.equal(tok[:, 0], torch.argmax(chain / q, -1)), "multinomial != argmax(p / exponential_)"
            if _ratio_margin(chain / q) < MARGIN or _ratio_margin(chain) < MARGIN:
                continue
            break
        else:
            raise RuntimeError("no seed with clear margins for %s %s" % (variant, kind))
        pre = kind + "/"
        rec[pre + "logits"], rec[pre + "flag"], rec[pre + "history"] = logits.numpy(), flag.numpy(), hist.numpy()
        rec[pre + "masked"] = masked.numpy()
        for k in ks:
            rec[pre + "topk_%d" % k] = top_k_logits(masked, k).numpy()
        probs = F.softmax(masked, dim=-1)
        rec[pre + "probs"] = probs.numpy()
        for p in ps:
            rec[pre + "topp_%g" % p] = top_p_logits(probs, p).numpy()
        rec[pre + "chain_k"], rec[pre + "chain_p"] = np.array(k0), np.array(p0)
        rec[pre + "chain_probs"] = chain.numpy()
        rec[pre + "q"] = q.numpy()
        rec[pre + "token_sample"] = tok.numpy()
        rec[pre + "token_greedy"] = torch.topk(chain, 1, dim=-1).indices.numpy()
        rec[pre + "ks"], rec[pre + "ps"] = np.array(ks), np.array(ps)
    for k, v in c.items():
        rec["code/" + k] = np.array(v)
    rec["variant"] = np.array(variant)
    np.savez_compressed(os.path.join(OUT, "sample_head_%s_%s.npz" % (variant, tag)), **rec)


def gen_transfer():
    c = codes_2026()
    B = 5
    g = torch.Generator().manual_seed(11)
    eos, pad, ncell = c["coarse_position_eos_code"], c["coarse_position_pad_code"], 256
    rows = []
    for b, n in enumerate((0, 7, 40, 255, 19)):
        pos = torch.randperm(ncell, generator=g)[:n]
        if n > 5:
            pos = torch.cat([pos, pos[:3]])                               # repeated positions
        after = torch.randperm(ncell, generator=g)[:4]                   # positions after the eos are ignored
        rows.append(torch.cat([torch.tensor([258 if b % 2 == 0 else 300 + b]), pos, torch.tensor([eos]), after]))
    L = max(r.numel() for r in rows) + 2
    cp = torch.full((B, L), pad, dtype=torch.long)
    for b, r in enumerate(rows):
        cp[b, :r.numel()] = r
    rec = {"coarse_position": cp.numpy()}
    for variant in ("class", "class2_entropy"):
        for order in ("region-first", "row-first"):
            m = _model(variant, c, order)
            rec["%s/%s/sampled" % (variant, order)] = m.transfer_sampled_coarse_position_to_sampled_fine_position(cp).numpy()
            rec["%s/%s/remain" % (variant, order)] = m.transfer_sampled_coarse_position_to_remain_fine_position(cp).numpy()
    for k, v in c.items():
        rec["code/" + k] = np.array(v)
    np.savez_compressed(os.path.join(OUT, "sample_transfer.npz"), **rec)


def gen_permuter():
    rec = {}
    c = codes_2026()
    for order in ("region-first", "row-first"):
        p = _permuter(order, 16, 32, c)
        for name in ("content_eos_tensor", "coarse_position_eos_tensor", "fine_position_eos_tensor", "position_sequence_coarse",
                     "position_sequence_fine"):
            rec["%s/%s" % (order, name)] = getattr(p, name).numpy()
    np.savez_compressed(os.path.join(OUT, "sample_permuter.npz"), **rec)


LOOP_CASES = [
    # name, variant, order, fix_fine_position, sample, temperature, (top_k, top_p, top_k_pos, top_p_pos)
    ("class_plain", "class", "region-first", False, True, 1.0, (None, None, None, None)),
    ("class_filters", "class", "region-first", False, True, 0.7, (5, 0.9, 8, 0.95)),
    ("class_fix", "class", "row-first", True, True, 1.0, (5, 0.9, None, None)),
    ("class_greedy", "class", "row-first", False, False, 1.0, (None, None, None, None)),
    ("class2_filters", "class2_entropy", "region-first", False, True, 1.0, (7, 0.85, 6, 0.9)),
    ("class2_fix_greedy", "class2_entropy", "region-first", True, False, 1.0, (None, None, None, None)),
    ("class2_plain_rowfirst", "class2_entropy", "row-first", False, True, 1.3, (None, None, None, None)),
    ("uncond_filters", "uncond", "region-first", False, True, 1.0, (5, 0.9, 8, 0.95)),
    ("uncond_fix_greedy", "uncond", "row-first", True, False, 1.0, (None, None, None, None)),
]


def gen_loop(B=4):
    c = R.codes_small()
    rec = {}
    mods = {v: _ref(v) for v in ("class", "class2_entropy", "uncond")}
    orig_mult, orig_topk = torch.multinomial, torch.topk
    for name, variant, order, fix, sample, temp, (tk, tp, kp, pp) in LOOP_CASES:
        mod = mods[variant]
        orig_topp = mod.top_p_logits
        for seed in range(2000):
            margins = {"ratio": 1.0, "greedy": 1.0, "cut": 1.0}

            def mult(probs, num_samples, *a, **kw):
                state = torch.get_rng_state()
                ix = orig_mult(probs, num_samples, *a, **kw)
                after = torch.get_rng_state()
                torch.set_rng_state(state)
                q = torch.empty_like(probs).exponential_(1)
                assert torch.equal(torch.argmax(probs / q, -1), ix[:, 0]) and torch.equal(torch.get_rng_state(), after)
                margins["ratio"] = min(margins["ratio"], _ratio_margin(probs / q))
                return ix

            def topk(x, k, *a, **kw):
                if k == 1 and x.shape[-1] > 1:
                    margins["greedy"] = min(margins["greedy"], _ratio_margin(x))
                return orig_topk(x, k, *a, **kw)

            def topp(probs, pv):
                margins["cut"] = min(margins["cut"], _cut_margin(probs, pv))
                return orig_topp(probs, pv)

            m = _model(variant, c, order, R.StubTransformer(c))
            torch.multinomial, torch.topk, mod.top_p_logits = mult, topk, topp
            try:
                torch.manual_seed(seed)
                out = m.sample_from_scratch(*R.conditioning(c, B), temperature=temp, sample=sample, top_k=tk, top_p=tp,
                                            top_k_pos=kp, top_p_pos=pp, process=False, fix_fine_position=fix)
            finally:
                torch.multinomial, torch.topk, mod.top_p_logits = orig_mult, orig_topk, orig_topp
            if margins["ratio"] > MARGIN and margins["greedy"] > MARGIN and margins["cut"] > CUT_MARGIN:
                break
        else:
            raise RuntimeError("no seed with clear margins for " + name)
        for key, t in zip(("coarse", "fine", "pos_coarse", "pos_fine"), out):
            rec["%s/%s" % (name, key)] = t.numpy()
        rec[name + "/seed"] = np.array(seed)
        rec[name + "/margins"] = np.array([margins["ratio"], margins["greedy"], margins["cut"]])
        print(name, "seed", seed, "coarse", tuple(out[0].shape), "fine", tuple(out[1].shape), "margins", margins)
    rec["B"] = np.array(B)
    np.savez_compressed(os.path.join(OUT, "sample_loop.npz"), **rec)


def main():
    for variant in ("class", "class2_entropy", "uncond"):
        gen_head(variant, R.codes_small(), "small")
        gen_head(variant, codes_2026(), "v2026", B=4)
    gen_transfer()
    gen_permuter()
    gen_loop()


if __name__ == "__main__":
    main()
