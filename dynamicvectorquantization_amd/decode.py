"""Codes -> the input of the decoder's conv_in as ONE kernel (csrc/decode_head.hip), the step after stage-2 sampling.

Reference: Dualformer.decode_to_img (models/stage2_dynamic/dqtransformer_uncond_entropy.py:174-178) runs permuter.forward_back,
first_stage_model.get_code_emb_with_depth (the codebook gather, channel-last), `.permute(0, 3, 1, 2)`, post_quant_conv (1x1) and
the position block of DecoderPositional.Decoder.forward (:109-118) before the decoder's conv_in.  All of it is a pure function
of (code, y, x):  h_in[b, c, y, x] = fl(fl(T[codes[b, y, x], c] + F[c, y, x]) + L[c, y, x])  with
  T = E W^T + b        post_quant_conv applied to every codebook row once (`dvq_decode_table_prepare_f32`)
  F, L                 the decoder's position biases, made by the decoder's OWN position modules, one table per module in the
                       order forward applies them, so the kernel's two adds round as the reference's two adds do

DecodeHead(quantize, post_quant_conv=None, decoder=None)   .from_codes(codes [B, H, W]) / .from_tokens(permuter, streams...)
FusedDecode                                                mixin: decode_to_img for the reference's Dualformer classes
Inference only (no autograd).  The tables are cached on (data_ptr, _version, shape, device) of the parameters they come from:
`load_state_dict`-style in-place copies and `.to()` are seen; a write through `.data` is not -- call `invalidate()` after one,
as for the codebook cache (VectorQuantize2.invalidate_codebook_cache).
"""
import torch
from torch import nn

from . import _lib
from ._prepared import PreparedImage

checked = _lib.checked

# Decoder.forward's dispatch on position_type (DecoderPositional.py:110-118), restated with its quirks: "learned" and
# "learned-relative" construct a position_bias that forward never applies
_NO_TABLE = ("learned", "learned-relative")


def _tensor_key(t):
    return None if t is None else (t.data_ptr(), t._version, tuple(t.shape), t.device)


def _position_modules(decoder):
    """[(kind, module)] in the order Decoder.forward applies them; () when the decoder adds no position bias"""
    if decoder is None or not hasattr(decoder, "position_type"):        # modules/dynamic_modules/Decoder.py: no position block
        return ()
    pt = decoder.position_type
    if pt == "fourier":
        return (("fourier", decoder.position_bias),)
    if pt == "fourier+learned":
        return (("fourier", decoder.position_bias_fourier), ("learned", decoder.position_bias_learned))
    if pt in _NO_TABLE:
        return ()
    raise NotImplementedError("decoder.position_type %r: the reference's Decoder constructor rejects it "
                              "(DecoderPositional.py:94-107)" % (pt,))


def _codebook_weight(quantize):
    """the weight tensor get_codebook_entry indexes: VQEmbedding's [K + 1, D] (padding row included), VectorQuantizer2's [K, D]"""
    if isinstance(quantize, nn.Embedding):
        return quantize.weight
    if getattr(quantize, "remap", None) is not None:
        raise NotImplementedError("DecodeHead: a remapped VectorQuantizer2 (get_codebook_entry translates the indices first)")
    for name in ("codebook", "embedding"):
        emb = getattr(quantize, name, None)
        if isinstance(emb, nn.Embedding):
            return emb.weight
    raise TypeError("DecodeHead: %s has no `codebook` / `embedding` nn.Embedding" % type(quantize).__name__)


class DecodeHead:
    """Holds no parameters: two prepared images made from the modules' parameters and rebuilt when those change."""

    def __init__(self, quantize, post_quant_conv=None, decoder=None):
        conv = post_quant_conv
        if conv is not None and not (isinstance(conv, nn.Conv2d) and tuple(conv.kernel_size) == (1, 1) and tuple(conv.stride) == (1, 1)
                                     and tuple(conv.padding) == (0, 0) and conv.groups == 1 and tuple(conv.dilation) == (1, 1)):
            raise TypeError("DecodeHead: post_quant_conv must be a plain 1x1 nn.Conv2d")
        self.quantize, self.post_quant_conv, self.decoder = quantize, conv, decoder
        weight = _codebook_weight(quantize)
        if conv is not None and conv.in_channels != weight.shape[1]:
            raise ValueError("post_quant_conv expects %d channels, the codebook has %d" % (conv.in_channels, weight.shape[1]))
        self.channels = weight.shape[1] if conv is None else conv.out_channels
        self._positions = _position_modules(decoder)                      # raises NotImplementedError for "relative" / "full"
        self._table = PreparedImage()
        self._pos = PreparedImage()

    def invalidate(self):
        """call after writing the codebook, the conv or the decoder's position parameters through `.data`"""
        self._table.invalidate()
        self._pos.invalidate()

    def _parameters(self):
        ps = [_codebook_weight(self.quantize)]
        if self.post_quant_conv is not None:
            ps += list(self.post_quant_conv.parameters())
        for _, m in self._positions:
            ps += list(m.parameters())
        return ps

    def _guard(self):
        if torch.is_grad_enabled() and any(p.requires_grad for p in self._parameters()):
            raise RuntimeError("DecodeHead is inference only (its kernel has no backward) and a parameter it reads requires grad: "
                               "call it under torch.no_grad(), or decode z_q with torch's conv when training")

    def table(self):
        """T [rows, C] float32 on the codebook's device: the codebook itself without a conv"""
        w = _codebook_weight(self.quantize)
        conv = self.post_quant_conv
        if not w.is_cuda:
            raise _lib.DvqError("the codebook is on %s: the dvq kernels run on the GPU only (no CPU fallback)" % w.device)
        if conv is None:
            return _lib.require_cuda_f32(w.detach(), "codebook")
        rows, D = w.shape
        C = conv.out_channels
        key = (_tensor_key(w), _tensor_key(conv.weight), _tensor_key(conv.bias))
        buf = self._table.lookup(key, w.device)
        if buf is None:
            e = _lib.require_cuda_f32(w.detach(), "codebook")
            cw = _lib.require_cuda_f32(conv.weight.detach().reshape(C, D), "post_quant_conv.weight")
            cb = None if conv.bias is None else _lib.require_cuda_f32(conv.bias.detach(), "post_quant_conv.bias")
            if cw.device != w.device:
                raise _lib.DvqError("post_quant_conv is on %s, the codebook on %s" % (cw.device, w.device))
            nbytes = checked.dvq_decode_table_bytes(rows, C)
            buf = self._table.rebuild(key, w.device, nbytes, lambda p, size, stream: checked.dvq_decode_table_prepare_f32(
                e.data_ptr(), rows, D, cw.data_ptr(), _lib.ptr(cb), C, p, size, stream))
        return buf[:rows * C * 4].view(torch.float32).view(rows, C)

    def position_tables(self, H, W, device):
        """(first, second): [C, H * W] float32 tables in application order, None where Decoder.forward adds nothing"""
        if not self._positions:
            return None, None
        C, n = self.channels, len(self._positions)
        key = (H, W, device) + tuple(_tensor_key(p) for _, m in self._positions for p in m.parameters())
        buf = self._pos.lookup(key, device)
        if buf is None:
            tabs = []
            for kind, m in self._positions:
                if any(p.device != device for p in m.parameters()):
                    raise _lib.DvqError("the decoder's position parameters are not on %s" % device)
                with torch.no_grad():
                    if kind == "fourier":                                 # FourierPositionEmbedding.forward: x + lff(coord)
                        t = m.lff(m.coord.to(device))
                    else:                                                 # PositionEmbedding2DLearned.forward: x + pos
                        t = m(torch.zeros((1, C, H, W), dtype=torch.float32, device=device))
                if tuple(t.shape) != (1, C, H, W) or t.dtype != torch.float32:
                    raise ValueError("the decoder's %s position bias is %s %s, the codes need (1, %d, %d, %d) float32"
                                     % (kind, tuple(t.shape), t.dtype, C, H, W))
                tabs.append(t.reshape(C * H * W))
            img = self._pos
            buf = img.rebuild(key, device, n * C * H * W * 4,
                              lambda p, size, stream: img.buf.view(torch.float32).copy_(torch.cat(tabs)))
        f = buf.view(torch.float32).view(n, C, H * W)
        return f[0], (f[1] if n > 1 else None)

    def from_codes(self, codes):
        """codes [B, H, W] int64 on the GPU -> h_in [B, C, H, W] float32, what decoder.conv_in reads"""
        self._guard()
        if not isinstance(codes, torch.Tensor):
            raise TypeError("codes must be a torch.Tensor")
        if not codes.is_cuda:
            raise _lib.DvqError("codes is on %s: the dvq kernels run on the GPU only (no CPU fallback)" % codes.device)
        if codes.dim() != 3:
            raise ValueError("codes must be [B, H, W], got %s" % (tuple(codes.shape),))
        if codes.dtype != torch.int64:
            codes = codes.long()
        codes = codes.contiguous()
        B, H, W = codes.shape
        dev = codes.device
        with _lib.on_device(dev):
            T = self.table()
            if T.device != dev:
                raise _lib.DvqError("codes is on %s, the codebook on %s" % (dev, T.device))
            rows, C = T.shape
            first, second = self.position_tables(H, W, dev)
            h_in = torch.empty((B, C, H, W), dtype=torch.float32, device=dev)
            if B * H * W:
                checked.dvq_decode_head_f32(codes.data_ptr(), B, H * W, T.data_ptr(), rows, C, _lib.ptr(first),
                                            _lib.ptr(second), h_in.data_ptr(), _lib.stream_ptr(dev))
        return h_in

    def from_tokens(self, permuter, coarse_content, fine_content, coarse_position, fine_position):
        """the permuter's forward_back (`dvq_permute_dual_backward_i64`), then from_codes: two launches, no host sync"""
        self._guard()
        return self.from_codes(permuter.forward_back(coarse_content, fine_content, coarse_position, fine_position))


class FusedDecode:
    """Mixin: decode_to_img through DecodeHead.  Put it first among the bases of a reference Dualformer (next to, or without,
    sample.FusedSampling).  The decoder is entered at conv_in through the integrator's cut of Decoder.forward
    (INTEGRATION.md): `forward(self, h, grain_indices, h_in=None)` skips post-conv input and position block when h_in is given."""

    def decode_head(self):
        fs = self.first_stage_model
        head = self.__dict__.get("_dvq_decode_head")
        if head is None or head.quantize is not fs.quantize or head.post_quant_conv is not fs.post_quant_conv \
                or head.decoder is not fs.decoder:
            head = DecodeHead(fs.quantize, fs.post_quant_conv, fs.decoder)
            self.__dict__["_dvq_decode_head"] = head
        return head

    @torch.no_grad()                                     # as the reference's own decode_to_img
    def decode_to_img(self, coarse_content, fine_content, coarse_position, fine_position):
        h_in = self.decode_head().from_tokens(self.permuter, coarse_content, fine_content, coarse_position, fine_position)
        return self.first_stage_model.decoder(None, None, h_in=h_in)
