"""Stage-2 generation glue on the GPU: the sampling step and the coarse -> fine position transfer of
Dualformer.sample_from_scratch (reference models/stage2_dynamic/dqtransformer_{class,class2_entropy,uncond_entropy}.py),
backed by csrc/sample.hip.  The transformer itself stays the caller's.

sample_step(logits, kind, rules, ...)   `[:, -1, :] / temperature`, the step's avoid_* mask, top_k_logits, softmax,
                                        top_p_logits and torch.multinomial / torch.topk as ONE kernel launch for all rows
transfer_sampled_coarse_position_to_{sampled,remain}_fine_position(model_or_rules, coarse_position, max_len=None)
                                        the reference methods of the same names: a count and a fill kernel
FusedSampling                           mixin whose sample_from_scratch makes the reference's transformer calls and
                                        replaces only the glue:  class Dualformer(FusedSampling, RefDualformer):
                                        sampling_variant = "class2_entropy"
The draw: torch.multinomial(p, 1) computes argmax(p / q) with q = empty_like(p).exponential_(1); sample_step draws q the
same way from `generator` (a CPU generator draws on the CPU and copies, so a seeded GPU run reproduces a seeded CPU run).
"""
import ctypes

import torch

from . import _lib

checked = _lib.checked

VARIANTS = ("class", "class2_entropy", "uncond")
KINDS = ("coarse_position", "fine_position", "content")
_NEG = -1


class SamplingRules:
    """The special codes of one model and the mask rule of each step kind (include/dvq.h, dvq_sample_head_f32).
    variant: "class" (dqtransformer_class.py), "class2_entropy" (dqtransformer_class2_entropy.py) or "uncond"
    (dqtransformer_uncond_entropy.py)."""

    def __init__(self, variant, *, content_pad_code, content_eos_code, coarse_position_pad_code, coarse_position_eos_code,
                 fine_position_pad_code, fine_position_eos_code, max_coarse_postion_idx, hw1, fine_hw, fine_position_order,
                 fine_position_sos_code=None, content_sos_code=None, activate_sos_for_fine_sequence=True):
        if variant not in VARIANTS:
            raise ValueError("variant %r: one of %s" % (variant, VARIANTS))
        if variant != "class2_entropy" and fine_position_sos_code is None:
            raise ValueError("variant %r bans fine_position_sos_code: it is required" % variant)
        if variant == "uncond" and content_sos_code is None:
            raise ValueError("variant 'uncond' bans content_sos_code: it is required")
        if fine_hw != 2 * hw1:
            raise NotImplementedError("fine_hw=%d, hw1=%d: the transfer serves fine_hw = 2 * hw1 (four fine positions per coarse "
                                      "cell, as the permuter)" % (fine_hw, hw1))
        if fine_position_order not in ("region-first", "row-first"):
            raise ValueError("fine_position_order %r" % (fine_position_order,))
        self.variant = variant
        self.content_pad_code, self.content_eos_code, self.content_sos_code = content_pad_code, content_eos_code, content_sos_code
        self.coarse_position_pad_code, self.coarse_position_eos_code = coarse_position_pad_code, coarse_position_eos_code
        self.fine_position_pad_code, self.fine_position_eos_code = fine_position_pad_code, fine_position_eos_code
        self.fine_position_sos_code = fine_position_sos_code
        self.max_coarse_postion_idx = max_coarse_postion_idx
        self.hw1, self.fine_hw, self.fine_position_order = hw1, fine_hw, fine_position_order
        self.activate_sos_for_fine_sequence = activate_sos_for_fine_sequence
        # {pad, ban_a, ban_from, restore, ban_b, ban_from_post, flag_code}
        cpe, fpe = coarse_position_eos_code, fine_position_eos_code
        codes = {
            "coarse_position": (coarse_position_pad_code, _NEG, max_coarse_postion_idx, cpe, _NEG, _NEG, cpe),
            "fine_position": ((fine_position_pad_code, _NEG, _NEG, fpe, _NEG, fpe + 1, fpe) if variant == "class2_entropy" else
                              (fine_position_pad_code, _NEG, _NEG, fpe, fine_position_sos_code, _NEG, fpe)),
            "content": ((content_pad_code, content_eos_code, _NEG, _NEG, content_sos_code, _NEG, _NEG) if variant == "uncond" else
                        (content_pad_code, _NEG, content_eos_code, _NEG, _NEG, _NEG, _NEG)),
        }
        self.codes = {k: tuple(int(c) for c in v) for k, v in codes.items()}
        self._c = {k: (ctypes.c_int64 * 7)(*v) for k, v in self.codes.items()}

    @classmethod
    def from_model(cls, model, variant=None):
        """read the attribute names the reference models set in __init__ (dqtransformer_class.py:52-70)"""
        variant = variant or getattr(model, "sampling_variant", None)
        if variant is None:
            raise ValueError("no variant given and the model has no `sampling_variant`")
        return cls(variant, content_pad_code=model.content_pad_code, content_eos_code=model.content_eos_code,
                   coarse_position_pad_code=model.coarse_position_pad_code,
                   coarse_position_eos_code=model.coarse_position_eos_code,
                   fine_position_pad_code=model.fine_position_pad_code, fine_position_eos_code=model.fine_position_eos_code,
                   max_coarse_postion_idx=model.max_coarse_postion_idx, hw1=model.hw1, fine_hw=model.fine_hw,
                   fine_position_order=model.fine_position_order,
                   fine_position_sos_code=getattr(model, "fine_position_sos_code", None),
                   content_sos_code=getattr(model, "content_sos_code", None),
                   activate_sos_for_fine_sequence=getattr(model, "activate_sos_for_fine_sequence", True))

    def sos_mode(self):
        if not self.activate_sos_for_fine_sequence:
            return _lib.TRANSFER_SOS_NONE
        return _lib.TRANSFER_SOS_COPY if self.variant == "class2_entropy" else _lib.TRANSFER_SOS_CONST


def _rules_of(model_or_rules):
    return model_or_rules if isinstance(model_or_rules, SamplingRules) else SamplingRules.from_model(model_or_rules)


def _cuda(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise _lib.DvqError("%s is on %s: the dvq kernels run on the GPU only (no CPU fallback)" % (name, t.device))
    return t


def draw_exponential(shape, device, generator=None):
    """q = Exp(1) draws of `shape`, consumed from `generator` exactly as torch.multinomial(p, 1) consumes it for p of that
    shape.  A CPU generator draws on the CPU (then one copy to `device`); None uses the device's default generator."""
    if generator is not None and generator.device.type == "cpu":
        return torch.empty(shape, dtype=torch.float32).exponential_(1, generator=generator).to(device)
    return torch.empty(shape, dtype=torch.float32, device=device).exponential_(1, generator=generator)


def sample_step(logits, kind, rules, history=None, flag=None, temperature=1.0, top_k=None, top_p=None, sample=True,
                generator=None, out=None, column=None, history_len=None, q=None, out_logits=None, out_probs=None):
    """One sampling step for all rows.  logits [B, T, V] (the last step is read in place) or [B, V], float32 on the GPU.
    kind: "coarse_position" | "fine_position" | "content"; rules: SamplingRules.  history: int64 [B, L] (the first
    history_len columns; position kinds only).  flag: float32 [B, 1] (or [B]), updated in place by += (token == eos) for
    the position kinds.  sample=True draws q (or takes the given [B, V] float32 q), else greedy.  out/column: write the
    token into out[:, column] (int64 [B, L]) and return that column as a [B, 1] view; otherwise a new [B, 1] tensor.
    out_logits / out_probs: optional float32 [B, V] tensors for the masked / top-k logits and the final probabilities.
    Token-only calls (q given or drawn on the device) do not synchronise and can be captured in a graph."""
    if kind not in KINDS:
        raise ValueError("kind %r: one of %s" % (kind, KINDS))
    _cuda(logits, "logits")
    if logits.dtype != torch.float32:
        raise _lib.DvqError("logits must be float32, got %s" % logits.dtype)
    if logits.dim() == 3:
        last = logits[:, -1, :]
    elif logits.dim() == 2:
        last = logits
    else:
        raise ValueError("logits must be [B, T, V] or [B, V], got %s" % (tuple(logits.shape),))
    if last.stride(-1) != 1:
        last = last.contiguous()
    B, V = last.shape
    dev = last.device
    if V > _lib.SAMPLE_MAX_V:
        raise _lib.DvqError("vocabulary V=%d exceeds the sampling head's limit %d" % (V, _lib.SAMPLE_MAX_V))
    if top_k is not None and top_k < 1:
        raise _lib.DvqError("top_k=%r must be >= 1" % (top_k,))
    if top_p is not None and not (0.0 < top_p <= 1.0):
        raise _lib.DvqError("top_p=%r outside (0, 1]" % (top_p,))
    if flag is None:
        flag = torch.zeros((B, 1), dtype=torch.float32, device=dev)
    _cuda(flag, "flag")
    if flag.dtype != torch.float32 or flag.numel() != B or not flag.is_contiguous():
        raise ValueError("flag must be a contiguous float32 [B, 1] tensor")
    hptr, hstride, hlen = 0, 0, 0
    if history is not None and kind != "content":
        _cuda(history, "history")
        if history.dtype != torch.int64 or history.dim() != 2 or history.shape[0] != B or history.stride(1) != 1:
            raise ValueError("history must be int64 [B, L] with unit column stride")
        hlen = history.shape[1] if history_len is None else int(history_len)
        hptr, hstride = history.data_ptr(), history.stride(0)
    if out is not None:
        _cuda(out, "out")
        if out.dtype != torch.int64 or out.dim() != 2 or out.shape[0] != B or column is None or not 0 <= column < out.shape[1]:
            raise ValueError("out must be int64 [B, L] with 0 <= column < L")
        ix = out[:, column:column + 1]
    else:
        ix = torch.empty((B, 1), dtype=torch.int64, device=dev)
    if sample:
        if q is None:
            q = draw_exponential((B, V), dev, generator)
        elif tuple(q.shape) != (B, V) or q.dtype != torch.float32 or not q.is_contiguous() or q.device != dev:
            raise ValueError("q must be a contiguous float32 [B, V] tensor on %s" % dev)
    for t, name in ((out_logits, "out_logits"), (out_probs, "out_probs")):
        if t is not None and (tuple(t.shape) != (B, V) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev):
            raise ValueError("%s must be a contiguous float32 [B, V] tensor on %s" % (name, dev))
    with _lib.on_device(dev):
        checked.dvq_sample_head_f32(last.data_ptr(), last.stride(0), B, V, float(temperature), rules._c[kind],
                                    hptr, hstride, hlen, flag.data_ptr(), int(top_k or 0), float(top_p or 0.0),
                                    1 if sample else 0, _lib.ptr(q) if sample else 0, ix.data_ptr(), ix.stride(0),
                                    _lib.ptr(out_logits), _lib.ptr(out_probs), _lib.stream_ptr(dev))
    return ix


def _transfer(model_or_rules, coarse_position, variant, max_len):
    r = _rules_of(model_or_rules)
    cp = _cuda(coarse_position, "coarse_position")
    if cp.dtype != torch.int64:
        cp = cp.long()
    if cp.dim() != 2 or cp.stride(1) != 1:
        cp = cp.contiguous()
    B, Lc = cp.shape
    dev = cp.device
    sos_mode = r.sos_mode()
    with _lib.on_device(dev):
        st = _lib.stream_ptr(dev)
        if max_len is None:
            counts = torch.empty(B, dtype=torch.int32, device=dev)
            mx = torch.empty(1, dtype=torch.int32, device=dev)
            checked.dvq_sample_transfer_count_i64(cp.data_ptr(), cp.stride(0), B, Lc, r.hw1, r.coarse_position_eos_code,
                                                  variant, counts.data_ptr(), mx.data_ptr(), st)
            L = (sos_mode != _lib.TRANSFER_SOS_NONE) + 4 * int(mx.item()) + 1      # the sync pad_sequence implies
        else:
            L = int(max_len)
            if L < 1:
                raise ValueError("max_len must be >= 1, got %r" % (max_len,))
        out = torch.empty((B, L), dtype=torch.int64, device=dev)
        order = 0 if r.fine_position_order == "region-first" else 1
        checked.dvq_sample_transfer_fill_i64(cp.data_ptr(), cp.stride(0), B, Lc, r.hw1, r.coarse_position_eos_code,
                                             variant, order, sos_mode, int(r.fine_position_sos_code or 0),
                                             r.fine_position_eos_code, r.fine_position_pad_code, L, out.data_ptr(), st)
    return out


def transfer_sampled_coarse_position_to_sampled_fine_position(model_or_rules, coarse_position, max_len=None):
    """the fine positions of the coarse cells sampled before each row's coarse EOS (dqtransformer_class.py:492-516).
    max_len: the width of the result (sos column included) instead of the batch maximum -- no host read; entries that do
    not fit are dropped"""
    return _transfer(model_or_rules, coarse_position, _lib.TRANSFER_SAMPLED, max_len)


def transfer_sampled_coarse_position_to_remain_fine_position(model_or_rules, coarse_position, max_len=None):
    """the fine positions of the coarse cells NOT sampled (dqtransformer_class.py:464-490); max_len as above"""
    return _transfer(model_or_rules, coarse_position, _lib.TRANSFER_REMAIN, max_len)


class _Seq:
    """a growing [B, n] int64 sequence in a preallocated buffer: view() is what torch.cat would have built"""

    def __init__(self, init, extra=64):
        B, n = init.shape
        self.buf = torch.empty((B, n + extra), dtype=torch.int64, device=init.device)
        self.buf[:, :n] = init
        self.n = n

    def view(self):
        return self.buf[:, :self.n]

    def slot(self):
        """(buffer, column) of the next entry; the caller writes it, then calls push()"""
        if self.n == self.buf.shape[1]:
            grown = torch.empty((self.buf.shape[0], 2 * self.buf.shape[1]), dtype=torch.int64, device=self.buf.device)
            grown[:, :self.n] = self.buf
            self.buf = grown
        return self.buf, self.n

    def push(self, col=None):
        if col is not None:
            self.slot()
            self.buf[:, self.n:self.n + 1] = col
        self.n += 1


class FusedSampling:
    """Mixin: sample_from_scratch with the fused glue.  Put it first among the bases of a reference Dualformer and set
    `sampling_variant` ("class", "class2_entropy", "uncond").  The transformer is called exactly as the reference calls it."""

    sampling_variant = "class"

    @torch.no_grad()                                     # as the reference's own sample_from_scratch
    def sample_from_scratch(self, c_coarse, c_fine, c_pos_coarse, c_pos_fine, c_seg_coarse, c_seg_fine,
                            temperature=1.0, sample=True, top_k=None, top_p=None, top_k_pos=None, top_p_pos=None, process=True,
                            fix_fine_position=False, generator=None):
        rules = SamplingRules.from_model(self, self.sampling_variant)
        if self.activate_sos_for_fine_sequence:
            x_fine, x_pos_fine, x_seg_fine = c_fine, c_pos_fine, c_seg_fine
        else:
            x_fine, x_pos_fine, x_seg_fine = c_fine[:, :0], c_pos_fine[:, :0], c_seg_fine[:, :0]
        batch_size, device = c_coarse.size(0), c_coarse.device
        xc, xpc, xsc = _Seq(c_coarse), _Seq(c_pos_coarse), _Seq(c_seg_coarse)
        xf, xpf, xsf = _Seq(x_fine), _Seq(x_pos_fine), _Seq(x_seg_fine)
        step = dict(temperature=temperature, sample=sample, generator=generator)

        def draw(logits, kind, seq, flag, k, p, history=None):
            buf, col = seq.slot()
            ix = sample_step(logits, kind, rules, history=history, flag=flag, top_k=k, top_p=p, out=buf, column=col, **step)
            seq.push()
            return ix

        flag = torch.zeros(batch_size, 1, device=device)
        while not torch.all(flag.bool()):
            position_hidden, position_logits = self.transformer.sample_coarse_position(
                coarse_content=xc.view(), coarse_position=xpc.view(), coarse_seg=xsc.view())
            draw(position_logits, "coarse_position", xpc, flag, top_k_pos, top_p_pos, history=xpc.view())
            _, content_logits = self.transformer.sample_coarse_content(
                coarse_content=None, coarse_position=xpc.view(), coarse_seg=None, position_hidden=position_hidden)
            draw(content_logits, "content", xc, flag, top_k, top_p)
            if self.activate_segment:
                xsc.push(0)
            if process:
                print("\r sampling coarse: {}".format(xc.n), end="")

        flag = torch.zeros(batch_size, 1, device=device)
        if not fix_fine_position:
            banned = _Seq(transfer_sampled_coarse_position_to_sampled_fine_position(rules, xpc.view()))
            while not torch.all(flag.bool()):
                position_hidden, position_logits = self.transformer.sample_fine_position(
                    coarse_content=xc.view(), fine_content=xf.view(), coarse_position=xpc.view(), fine_position=xpf.view(),
                    coarse_seg=xsc.view(), fine_seg=xsf.view())
                ix_pos = draw(position_logits, "fine_position", xpf, flag, top_k_pos, top_p_pos, history=banned.view())
                banned.push(ix_pos)
                _, content_logits = self.transformer.sample_fine_content(
                    coarse_content=xc.view(), fine_content=xf.view(), coarse_position=xpc.view(), fine_position=xpf.view(),
                    coarse_seg=xsc.view(), fine_seg=xsf.view(), position_hidden=position_hidden)
                draw(content_logits, "content", xf, flag, top_k, top_p)
                if self.activate_segment:
                    xsf.push(1)
                if process:
                    print("\r sampled coarse size: {} ; sampling fine: {}".format(xc.n, xf.n), end="")
        else:
            remain = transfer_sampled_coarse_position_to_remain_fine_position(rules, xpc.view())
            for fine_index in range(remain.size(1)):
                if self.activate_sos_for_fine_sequence and fine_index == 0:
                    continue
                ix_pos = remain[:, fine_index].unsqueeze(-1)
                xpf.push(ix_pos)
                flag += (ix_pos == rules.fine_position_eos_code)
                _, content_logits = self.transformer.sample_fine_content(
                    coarse_content=xc.view(), fine_content=xf.view(), coarse_position=xpc.view(), fine_position=xpf.view(),
                    coarse_seg=xsc.view(), fine_seg=xsf.view(), position_hidden=None)
                draw(content_logits, "content", xf, flag, top_k, top_p)
                if self.activate_segment:
                    xsf.push(1)
                if process:
                    print("\r sampled coarse size: {} ; sampling fine: {}".format(xc.n, xf.n), end="")

        x_coarse = xc.view()[:, c_coarse.shape[1]:]
        x_pos_coarse = xpc.view()[:, c_pos_coarse.shape[1]:]
        x_fine, x_pos_fine = xf.view(), xpf.view()
        if self.activate_sos_for_fine_sequence:
            x_fine = x_fine[:, c_fine.shape[1]:]
            x_pos_fine = x_pos_fine[:, c_fine.shape[1]:]
        return x_coarse, x_fine, x_pos_coarse, x_pos_fine
