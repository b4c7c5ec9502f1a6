"""Test-side restatement of stage-2 sampling (reference models/stage2_dynamic/dqtransformer_*.py, models/stage2/utils.py) in
vectorised torch ops, plus the stub transformer the whole-loop goldens use.  Device-agnostic: the CPU tests check it against
the goldens, the GPU tests run it next to the kernels.  Imports no reference code."""
from types import SimpleNamespace

import numpy as np
import torch

NEG = -float("inf")


def codes_small():
    """the special codes of the small stub model: coarse 4 x 4, fine 8 x 8, a 32-entry codebook, 6 class labels"""
    return dict(content_pad_code=32, content_eos_code=33, content_sos_code=34, coarse_position_pad_code=16,
                coarse_position_eos_code=17, coarse_position_sos_code=18, fine_position_pad_code=64, fine_position_eos_code=65,
                fine_position_sos_code=66, max_coarse_postion_idx=15, hw1=4, fine_hw=8, V_content=40, V_coarse=19, V_fine=67)


def codes_for(V, hw1, layout="top"):
    """special codes for one vocabulary size V (all three step kinds share it) and a coarse grid hw1 x hw1.
    "top":    pad, eos, sos = V - 3, V - 2, V - 1 and max_coarse_postion_idx = V - 3, as the real models (positions below,
              special codes above); with V >= 4 * hw1 * hw1 + 3 no code collides with a coarse or fine position.
    "spread": one special code at index 0, one at 31 or 32 (the edge of a 32-bit word of the history bitmap) and one at
              V - 1; the coarse position range is banned from 3 V / 4 on, so the coarse eos (V - 1) is restored out of it.
    Below V = 4 there is no room for three codes: some coincide, chosen so that every unflagged row keeps a finite entry.
    Every code meets the range rules of dvq_sample_head_f32 (pad in [0, V), ban ranges in [0, V], the others in [0, V))."""
    V, hw1 = int(V), int(hw1)
    if V < 2:
        raise ValueError("V=%d: a vocabulary needs a pad code and one more entry" % V)
    if layout not in ("top", "spread"):
        raise ValueError("layout %r" % (layout,))
    if V == 2:                                           # index 0 stays finite: position eos = 0, content bans 1 only
        coarse = fine = (1, 0, 1)
        content, max_idx = (1, 1, 1), 1
    elif V == 3:
        coarse = fine = content = (1, 2, 1)
        max_idx = 1
    elif layout == "top":
        coarse = fine = content = (V - 3, V - 2, V - 1)
        max_idx = V - 3
    else:
        m31, m32 = (31, 32) if V > 33 else (V // 2, V // 2)
        coarse = (0, V - 1, m31)
        fine = (m32, V - 1, 0)
        content = (0, V - 1, m31)                        # content bans from eos on: eos stays at the top
        max_idx = max(3 * V // 4, 2)
    return dict(content_pad_code=content[0], content_eos_code=content[1], content_sos_code=content[2],
                coarse_position_pad_code=coarse[0], coarse_position_eos_code=coarse[1], coarse_position_sos_code=coarse[2],
                fine_position_pad_code=fine[0], fine_position_eos_code=fine[1], fine_position_sos_code=fine[2],
                max_coarse_postion_idx=max_idx, hw1=hw1, fine_hw=2 * hw1, V_content=V, V_coarse=V, V_fine=V)


def mask(logits, kind, variant, c, history, flag):
    """the avoid_* helper of the step kind (logits already divided by the temperature)"""
    B, V = logits.shape
    out = logits.clone()
    cols = torch.arange(V, device=logits.device)
    ban = torch.zeros_like(out, dtype=torch.bool)
    restore, post = None, torch.zeros(V, dtype=torch.bool, device=logits.device)
    if kind == "coarse_position":
        pad, eos = c["coarse_position_pad_code"], c["coarse_position_eos_code"]
        ban[:, pad] = True
        ban[:, c["max_coarse_postion_idx"]:] = True
        restore = eos
    elif kind == "fine_position":
        pad, eos = c["fine_position_pad_code"], c["fine_position_eos_code"]
        ban[:, pad] = True
        restore = eos
        if variant == "class2_entropy":
            post = cols >= eos + 1
        else:
            post = cols == c["fine_position_sos_code"]
    else:
        pad, eos = c["content_pad_code"], c["content_eos_code"]
        ban[:, pad] = True
        if variant == "uncond":
            ban[:, eos] = True
            ban[:, c["content_sos_code"]] = True
        else:
            ban[:, eos:] = True
    if history is not None and kind != "content":
        h = history[:, :]
        ok = (h >= 0) & (h < V)
        ban.scatter_(1, torch.where(ok, h, torch.full_like(h, pad)), True)
    out[ban] = NEG
    if restore is not None:
        out[:, restore] = logits[:, restore]
    out[:, post] = NEG
    flagged = flag.view(-1) != 0
    enforced = torch.full_like(out, NEG)
    enforced[:, pad] = logits[:, pad]
    return torch.where(flagged[:, None], enforced, out)


def top_k(logits, k):
    kth = torch.topk(logits, k, dim=-1).values[:, -1:]
    return torch.where(logits < kth, torch.full_like(logits, NEG), logits)


def top_p(probs, p):
    """keep an element iff the mass strictly before it (p descending, index ascending) is < p; renormalise"""
    order = torch.sort(probs, dim=-1, descending=True, stable=True).indices
    sp = torch.gather(probs, -1, order)
    before = torch.cumsum(sp, dim=-1) - sp
    keep_sorted = before < p
    keep_sorted[:, 0] = True
    keep = torch.zeros_like(keep_sorted).scatter(-1, order, keep_sorted)
    kept = torch.where(keep, probs, torch.zeros_like(probs))
    return kept / kept.sum(-1, keepdim=True)


def softmax64(masked32):
    """float64 softmax of float32 masked logits.  The row maximum is subtracted in float32, as the kernel does: that
    difference is one IEEE operation and the same on every device, so exp and the normalisation are the only things a
    float32 softmax can get wrong against this.  Returns a float64 tensor."""
    assert masked32.dtype == torch.float32
    d = masked32 - masked32.max(dim=-1, keepdim=True).values
    e = torch.exp(d.double())
    return e / e.sum(-1, keepdim=True)


def top_p_exact(p32, top_p):
    """top_p_logits on float32 probabilities with float64 masses.  Order: value descending, index ascending (a stable sort).
    An element is kept iff the mass strictly before it is < float32(top_p); the first element is always kept.
    Returns (keep bool [B, V], float64 [B, V] kept values renormalised, margin float64 [B]): margin is the per-row minimum of
    |mass before j - top_p| over the elements with p > 0 (whether an element of probability 0 counts as kept changes neither
    the set of non-zero outputs nor their sum).  A row whose margin is above the error of the masses being compared has one
    correct kept set."""
    p = np.ascontiguousarray(p32.detach().cpu().numpy())
    assert p.dtype == np.float32 and p.ndim == 2
    t = float(np.float32(top_p))
    p64 = p.astype(np.float64)
    order = np.argsort(-p64, axis=-1, kind="stable")
    sp = np.take_along_axis(p64, order, -1)
    before = np.concatenate([np.zeros_like(sp[:, :1]), np.cumsum(sp, -1)[:, :-1]], -1)
    keep_sorted = before < t
    keep_sorted[:, 0] = True
    keep = np.zeros_like(keep_sorted)
    np.put_along_axis(keep, order, keep_sorted, -1)
    kept = np.where(keep, p64, 0.0)
    margin = np.where(sp > 0, np.abs(before - t), np.inf).min(-1)
    return torch.from_numpy(keep), torch.from_numpy(kept / kept.sum(-1, keepdims=True)), torch.from_numpy(margin)


def head(logits_last, kind, variant, c, history, flag, temperature, k, p, sample, generator):
    x = logits_last / temperature
    x = mask(x, kind, variant, c, history, flag)
    if k is not None:
        x = top_k(x, k)
    probs = torch.softmax(x, dim=-1)
    if p is not None:
        probs = top_p(probs, p)
    if sample:
        return torch.multinomial(probs, 1, generator=generator)
    return torch.topk(probs, 1, dim=-1).indices


def transfer_selected(c, coarse_position, remain):
    """bool [B, hw1 * hw1]: the coarse cells whose fine positions the transfer emits (sampled before the row's first coarse
    EOS, or with `remain` the others).  Column 0 is the sos; a row of that column alone has sampled nothing."""
    hw1 = c["hw1"]
    B, Lc = coarse_position.shape
    dev = coarse_position.device
    cp = coarse_position[:, 1:]
    is_eos = cp == c["coarse_position_eos_code"]
    first = torch.full((B,), Lc - 1, device=dev)
    if Lc > 1:                                           # argmax over an empty dimension raises
        first = torch.where(is_eos.any(1), is_eos.float().argmax(1), first)
    valid = (torch.arange(Lc - 1, device=dev)[None, :] < first[:, None]) & (cp >= 0) & (cp < hw1 * hw1)
    mark = torch.zeros((B, hw1 * hw1 + 1), dtype=torch.bool, device=dev)
    mark.scatter_(1, torch.where(valid, cp, torch.full_like(cp, hw1 * hw1)), True)
    return mark[:, :-1] != bool(remain)


def transfer(c, coarse_position, remain, order, sos_mode):
    """sos_mode: "const" (fine_position_sos_code), "copy" (coarse_position[:, 0]) or None"""
    hw1, fine_hw = c["hw1"], c["fine_hw"]
    B = coarse_position.shape[0]
    dev = coarse_position.device
    sel = transfer_selected(c, coarse_position, remain)
    seq = torch.arange(fine_hw * fine_hw, device=dev).view(fine_hw, fine_hw)
    if order == "region-first":
        seq = seq.view(hw1, 2, hw1, 2).permute(0, 2, 1, 3).reshape(hw1 * hw1, 4)
        rows = [seq[sel[b]].reshape(-1) for b in range(B)]
    else:
        fine_sel = sel.view(B, hw1, hw1).repeat_interleave(2, -1).repeat_interleave(2, -2)
        rows = [seq[fine_sel[b]] for b in range(B)]
    n = max(int(r.numel()) for r in rows) + 1
    out = torch.full((B, n), c["fine_position_pad_code"], dtype=torch.long, device=dev)
    for b, r in enumerate(rows):
        out[b, :r.numel()] = r
        out[b, r.numel()] = c["fine_position_eos_code"]
    if sos_mode == "const":
        out = torch.cat([torch.full((B, 1), c["fine_position_sos_code"], dtype=torch.long, device=dev), out], 1)
    elif sos_mode == "copy":
        out = torch.cat([coarse_position[:, :1], out], 1)
    return out


class StubTransformer:
    """logits = a gather from a fixed float32 table, keyed by integer hashes of the inputs: bit-identical on every device"""

    def __init__(self, c, seed=7, rows=97, scale=3.0):
        g = np.random.default_rng(seed)
        self.rows = rows
        self.t = {k: torch.from_numpy((g.standard_normal((rows, c[k])) * scale).astype(np.float32))
                  for k in ("V_coarse", "V_content", "V_fine")}

    def _tab(self, key, ref):
        return self.t[key].to(ref.device)

    def _hash(self, *seqs):
        h = None
        for i, s in enumerate(seqs):
            if s is None or s.shape[1] == 0:
                continue
            w = torch.arange(1, s.shape[1] + 1, device=s.device, dtype=torch.long) * (7 + 4 * i)
            v = (s.long() * w).sum(1) + 13 * s.shape[1]
            h = v if h is None else h * 31 + v
        return h % self.rows

    def sample_coarse_position(self, coarse_content, coarse_position, coarse_seg):
        k = self._hash(coarse_content, coarse_position)
        return k, self._tab("V_coarse", k)[k][:, None, :]

    def sample_coarse_content(self, coarse_content=None, coarse_position=None, coarse_seg=None, position_hidden=None):
        k = (position_hidden * 5 + coarse_position[:, -1] * 11) % self.rows
        return None, self._tab("V_content", k)[k][:, None, :]

    def sample_fine_position(self, coarse_content, fine_content, coarse_position, fine_position, coarse_seg, fine_seg):
        k = self._hash(coarse_content, coarse_position, fine_content, fine_position)
        return k, self._tab("V_fine", k)[k][:, None, :]

    def sample_fine_content(self, coarse_content, fine_content, coarse_position, fine_position, coarse_seg, fine_seg,
                            position_hidden=None):
        if position_hidden is None:
            position_hidden = self._hash(fine_content, coarse_content)
        k = (position_hidden * 3 + fine_position[:, -1] * 17) % self.rows
        return None, self._tab("V_content", k)[k][:, None, :]


def model_attrs(c, variant, order, activate_segment=True):
    a = dict(content_pad_code=c["content_pad_code"], content_eos_code=c["content_eos_code"],
             coarse_position_pad_code=c["coarse_position_pad_code"], coarse_position_eos_code=c["coarse_position_eos_code"],
             fine_position_pad_code=c["fine_position_pad_code"], fine_position_eos_code=c["fine_position_eos_code"],
             max_coarse_postion_idx=c["max_coarse_postion_idx"], hw1=c["hw1"], hw2=2, fine_hw=c["fine_hw"],
             fine_position_order=order, activate_sos_for_fine_sequence=True, activate_segment=activate_segment)
    if variant != "class2_entropy":
        a["fine_position_sos_code"] = c["fine_position_sos_code"]
    if variant == "uncond":
        a["content_sos_code"] = c["content_sos_code"]
    return a


def conditioning(c, B, device="cpu"):
    """the class-conditional start: one class-label sos per sequence (coarse content / position, fine position)"""
    z = lambda v: torch.full((B, 1), v, dtype=torch.long, device=device)
    labels = torch.arange(B, device=device)[:, None] % 6 + 34
    return (labels, labels.clone(), z(c["coarse_position_sos_code"]), z(c["fine_position_sos_code"]), z(0), z(1))


def sample_loop(m, variant, c, cond, temperature=1.0, sample=True, top_k_=None, top_p_=None, top_k_pos=None, top_p_pos=None,
                fix_fine_position=False, generator=None):
    """the reference loop (dqtransformer_class.py:299-461) with the restated glue; m: attributes + transformer"""
    c_coarse, c_fine, c_pos_coarse, c_pos_fine, c_seg_coarse, c_seg_fine = cond
    x_coarse, x_fine, x_pos_coarse, x_pos_fine, x_seg_coarse, x_seg_fine = cond
    B, dev = x_coarse.size(0), x_coarse.device
    order = m.fine_position_order
    sos = "copy" if variant == "class2_entropy" else "const"
    hd = lambda lg, kind, hist, flag, k, p: head(lg[:, -1, :], kind, variant, c, hist, flag, temperature, k, p, sample, generator)
    flag = torch.zeros(B, 1, device=dev)
    while not torch.all(flag.bool()):
        ph, pl = m.transformer.sample_coarse_position(coarse_content=x_coarse, coarse_position=x_pos_coarse, coarse_seg=x_seg_coarse)
        ix_pos = hd(pl, "coarse_position", x_pos_coarse, flag, top_k_pos, top_p_pos)
        x_pos_coarse = torch.cat((x_pos_coarse, ix_pos), 1)
        flag = flag + (ix_pos == c["coarse_position_eos_code"])
        _, cl = m.transformer.sample_coarse_content(coarse_content=None, coarse_position=x_pos_coarse, coarse_seg=None, position_hidden=ph)
        ix = hd(cl, "content", None, flag, top_k_, top_p_)
        x_seg_coarse = torch.cat([x_seg_coarse, torch.zeros(B, 1, dtype=torch.long, device=dev)], 1)
        x_coarse = torch.cat((x_coarse, ix), 1)
    flag = torch.zeros(B, 1, device=dev)
    if not fix_fine_position:
        tf = transfer(c, x_pos_coarse, False, order, sos)
        while not torch.all(flag.bool()):
            ph, pl = m.transformer.sample_fine_position(coarse_content=x_coarse, fine_content=x_fine, coarse_position=x_pos_coarse,
                                                        fine_position=x_pos_fine, coarse_seg=x_seg_coarse, fine_seg=x_seg_fine)
            ix_pos = hd(pl, "fine_position", tf, flag, top_k_pos, top_p_pos)
            x_pos_fine = torch.cat((x_pos_fine, ix_pos), 1)
            tf = torch.cat([tf, ix_pos], 1)
            flag = flag + (ix_pos == c["fine_position_eos_code"])
            _, cl = m.transformer.sample_fine_content(coarse_content=x_coarse, fine_content=x_fine, coarse_position=x_pos_coarse,
                                                      fine_position=x_pos_fine, coarse_seg=x_seg_coarse, fine_seg=x_seg_fine,
                                                      position_hidden=ph)
            ix = hd(cl, "content", None, flag, top_k_, top_p_)
            x_fine = torch.cat((x_fine, ix), 1)
            x_seg_fine = torch.cat([x_seg_fine, torch.ones(B, 1, dtype=torch.long, device=dev)], 1)
    else:
        rem = transfer(c, x_pos_coarse, True, order, sos)
        for fi in range(1, rem.size(1)):
            ix_pos = rem[:, fi].unsqueeze(-1)
            x_pos_fine = torch.cat((x_pos_fine, ix_pos), 1)
            flag = flag + (ix_pos == c["fine_position_eos_code"])
            _, cl = m.transformer.sample_fine_content(coarse_content=x_coarse, fine_content=x_fine, coarse_position=x_pos_coarse,
                                                      fine_position=x_pos_fine, coarse_seg=x_seg_coarse, fine_seg=x_seg_fine,
                                                      position_hidden=None)
            ix = hd(cl, "content", None, flag, top_k_, top_p_)
            x_fine = torch.cat((x_fine, ix), 1)
            x_seg_fine = torch.cat([x_seg_fine, torch.ones(B, 1, dtype=torch.long, device=dev)], 1)
    return (x_coarse[:, c_coarse.shape[1]:], x_fine[:, c_fine.shape[1]:], x_pos_coarse[:, c_pos_coarse.shape[1]:],
            x_pos_fine[:, c_fine.shape[1]:])


def namespace(c, variant, order, seed=7):
    ns = SimpleNamespace(**model_attrs(c, variant, order))
    ns.transformer = StubTransformer(c, seed)
    return ns
