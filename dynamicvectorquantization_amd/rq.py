"""Residual quantization on the HIP assign path: a drop-in for the reference's RQBottleneck
(modules/vector_quantization/quantize_rqvae.py:149-400, built by models/stage1/rqvae.py:70-81).

Constructor arguments, attributes, `ValueError`s and state_dict keys are the reference's, so its checkpoints load; the codebooks
are this package's `VQEmbedding` (the reference's RQ codebook class is quantize2_mask.py's line for line).  Per depth i the forward
runs, in order:
  1. the flat assign on the residual r_i (`dvq_vq_assign_flat_f32`, codes only, with that codebook's cached prep): the
     reference's argmin bit for bit;
  2. `dvq_rq_step_f32`: agg / residual / loss partial / gradient sum / codes[:, i] (and on the last depth the straight-through
     output in latent layout) in one streaming pass;
  3. in training only, that codebook's EMA update on (r_i, c_i) (`VQEmbedding._ema_step` on the residual rows: the row-major
     statistics kernel and `dvq_ema_update_f32`), so with
     `shared_codebook=True` depth i + 1 searches the codebook depth i has just updated, as in the reference.
then `dvq_rq_loss_f32`.  Codes and `out` equal the reference bit for bit, the loss to 1e-5 relative.  The backward is one kernel
(`dvq_rq_backward_f32`); the codebooks, EMA buffers, get no gradient, as in the reference.
"""
import ctypes

import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from . import _lib
from .quantize import VQEmbedding, _wide_width, soft_assign, vq_assign

try:
    from collections.abc import Iterable
except ImportError:                                   # pragma: no cover
    from typing import Iterable

checked = _lib.checked


class _RQGeom:
    """the shapes of one call: x [B, H, W, Dl] latent, code grid h x w, D = rH rW Dl channels per token, N = B h w tokens"""
    __slots__ = ("B", "h", "w", "rH", "rW", "Dl", "D", "N", "depth")

    def __init__(self, mod, x):
        if x.dim() != 4:
            raise ValueError("RQBottleneck expects x [B, H, W, D] (channel-last latents), got %s" % (tuple(x.shape),))
        B, H, W, Dl = x.shape
        rH, rW = int(mod.shape_divisor[0]), int(mod.shape_divisor[1])
        if H % rH or W % rW or Dl != mod.latent_shape[2]:
            raise ValueError("latent %s does not fit latent_shape %s / code_shape %s"
                             % (tuple(x.shape[1:]), tuple(mod.latent_shape), tuple(mod.code_shape)))
        self.B, self.h, self.w, self.rH, self.rW, self.Dl = B, H // rH, W // rW, rH, rW, Dl
        self.D = rH * rW * Dl
        self.N = B * self.h * self.w
        self.depth = int(mod.code_shape[-1])
        _wide_width(self.D, "RQBottleneck")           # DvqError for widths the residual kernels do not serve
        if self.depth > _lib.RQ_MAX_DEPTH:
            raise _lib.DvqError("RQBottleneck: depth %d above the kernels' limit %d" % (self.depth, _lib.RQ_MAX_DEPTH))

    def args(self):
        return self.B, self.h, self.w, self.rH, self.rW, self.Dl, self.D


def _books(mod, depth):
    return [mod.codebooks[0] if mod.shared_codebook else mod.codebooks[i] for i in range(depth)]


def _rq_forward(mod, x, want_grad, want_loss, training, assign=None):
    """the per-depth loop of the module docstring -> (out, loss or None, codes, workspace).  `assign(i, codebook, r_i)` ->
    codes [N] (get_soft_codes) replaces the hard assign of each depth."""
    g = _RQGeom(mod, x)
    x = _lib.require_cuda_f32(x, "x")
    dev = x.device
    depth, N, D = g.depth, g.N, g.D
    out = torch.empty_like(x)
    codes = torch.empty((g.B, g.h, g.w, depth), dtype=torch.int64, device=dev)
    loss = torch.empty((), dtype=torch.float32, device=dev) if want_loss else None
    if N == 0:
        if loss is not None:
            loss.fill_(float("nan"))
        return out, loss, codes, None
    nbytes = checked.dvq_rq_workspace_bytes(N, D, depth, int(want_grad))
    if nbytes == 0:
        raise _lib.DvqError("RQBottleneck: unsupported shape N=%d D=%d depth=%d" % (N, D, depth))
    if want_grad:
        # the backward reads s from the workspace of ITS forward: one per call, kept on the autograd ctx
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    else:
        key = (dev, _lib.stream_ptr(dev), N, D, depth)
        ws = mod._ws.get(key)
        if ws is None:
            if len(mod._ws) >= 8:
                mod._ws.clear()
            ws = mod._ws[key] = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if g.rH == 1 and g.rW == 1:
        r = x.view(N, D)                              # the reference RQ-VAE configuration: no copy of x
    else:                                             # to_code_shape (:216-224): one code-layout copy for depth 0's search
        r = x.reshape(g.B, g.h, g.rH, g.w, g.rW, g.Dl).permute(0, 1, 3, 2, 4, 5).reshape(N, D)
    c = torch.empty(N, dtype=torch.int64, device=dev)
    stream = _lib.stream_ptr(dev)
    books = _books(mod, depth)
    with _lib.on_device(dev):
        for i, cb in enumerate(books):
            if training:
                cb._prep.invalidate()                 # training: optimizers / EMA may write through .data
            cb._prep.track_users = training
            weight = cb.weight
            if not (weight.is_cuda and weight.dtype == torch.float32 and weight.is_contiguous()):
                raise _lib.DvqError("RQBottleneck: codebook %d must be a contiguous f32 tensor on the GPU" % i)
            if assign is None:
                vq_assign(r, weight[:-1], cb._prep, want_zq=False, want_loss=False, mode=mod.assign_mode, out=(None, c, None))
            else:
                c = assign(i, cb, r)
            if training:
                cb._prep.used(dev)
            checked.dvq_rq_step_f32(
                x.data_ptr(), r.data_ptr(), weight.data_ptr(), cb.n_embed, c.data_ptr(), *g.args(), i, depth, int(want_grad),
                codes.data_ptr(), out.data_ptr(), ws.data_ptr(), ws.numel(), stream)
            if training and cb.ema:
                with torch.no_grad():
                    cb._ema_step(r, c)
            if i + 1 < depth:
                off = checked.dvq_rq_residual_offset(N, D, depth, i + 1)
                r = ws[off:off + N * D * 4].view(torch.float32).view(N, D)
        if loss is not None:
            checked.dvq_rq_loss_f32(N, D, depth, ws.data_ptr(), ws.numel(), loss.data_ptr(), stream)
    return out, loss, codes, ws


class _RQFunction(torch.autograd.Function):
    """forward = the per-depth kernel loop; backward = d out / d x (identity, the straight-through add) plus d loss / d x
    (`dvq_rq_backward_f32`: g_out + g_loss 2 / (numel d) sum_i (x - agg_{i+1}))"""

    @staticmethod
    def forward(ctx, x, mod, training):
        out, loss, codes, ws = _rq_forward(mod, x, True, True, training)
        ctx.ws, ctx.geom, ctx.device = ws, _RQGeom(mod, x), x.device
        ctx.mark_non_differentiable(codes)
        return out, loss, codes

    @staticmethod
    def backward(ctx, g_out, g_loss, _g_codes):
        g, ws = ctx.geom, ctx.ws
        gx = torch.empty((g.B, g.h * g.rH, g.w * g.rW, g.Dl), dtype=torch.float32, device=ctx.device)
        if ws is None:                                # empty batch
            return gx, None, None
        go = None if g_out is None else _lib.require_cuda_f32(g_out, "grad of out")
        gl = None if g_loss is None else g_loss.reshape(1).to(torch.float32).contiguous()
        with _lib.on_device(gx.device):
            checked.dvq_rq_backward_f32(
                _lib.ptr(go), _lib.ptr(gl), *g.args(), g.depth, ws.data_ptr(), ws.numel(), gx.data_ptr(),
                _lib.stream_ptr(gx.device))
        ctx.ws = None
        return gx, None, None


class RQBottleneck(nn.Module):
    """Reference quantize_rqvae.py:149-400.  x [B, H, W, D] channel-last -> (out [B, H, W, D], commitment loss, codes
    [B, h, w, d] int64).  `assign_mode` selects the assign path (MODE_FILTER, default, or MODE_EXACT: the same codes)."""

    def __init__(self,
                 latent_shape,
                 code_shape,
                 n_embed,
                 decay=0.99,
                 shared_codebook=False,
                 restart_unused_codes=True,
                 commitment_loss='cumsum'
                 ):
        super().__init__()
        if not len(code_shape) == len(latent_shape) == 3:
            raise ValueError("incompatible code shape or latent shape")
        if any([y % x != 0 for x, y in zip(code_shape[:2], latent_shape[:2])]):
            raise ValueError("incompatible code shape or latent shape")
        # residual quantization does not divide the feature dims (:194)
        embed_dim = np.prod(latent_shape[:2]) // np.prod(code_shape[:2]) * latent_shape[2]
        self.latent_shape = torch.Size(latent_shape)
        self.code_shape = torch.Size(code_shape)
        self.shape_divisor = torch.Size([latent_shape[i] // code_shape[i] for i in range(len(latent_shape))])
        self.shared_codebook = shared_codebook
        if self.shared_codebook:
            if isinstance(n_embed, Iterable) or isinstance(decay, Iterable):
                raise ValueError("Shared codebooks are incompatible \
                                    with list types of momentums or sizes: Change it into int")
        self.restart_unused_codes = restart_unused_codes
        self.n_embed = n_embed if isinstance(n_embed, Iterable) else [n_embed for _ in range(self.code_shape[-1])]
        self.decay = decay if isinstance(decay, Iterable) else [decay for _ in range(self.code_shape[-1])]
        assert len(self.n_embed) == self.code_shape[-1]
        assert len(self.decay) == self.code_shape[-1]
        if self.shared_codebook:
            codebook0 = VQEmbedding(self.n_embed[0], embed_dim, decay=self.decay[0], restart_unused_codes=restart_unused_codes)
            self.codebooks = nn.ModuleList([codebook0 for _ in range(self.code_shape[-1])])
        else:
            self.codebooks = nn.ModuleList([VQEmbedding(self.n_embed[i], embed_dim, decay=self.decay[i],
                                                        restart_unused_codes=restart_unused_codes)
                                            for i in range(self.code_shape[-1])])
        self.commitment_loss = commitment_loss
        self.assign_mode = _lib.MODE_FILTER
        self._ws = {}                                 # (device, stream, N, D, depth) -> inference workspace

    def to_code_shape(self, x):
        (B, H, W, D) = x.shape
        (rH, rW, _) = self.shape_divisor
        return x.reshape(B, H // rH, rH, W // rW, rW, D).permute(0, 1, 3, 2, 4, 5).reshape(B, H // rH, W // rW, -1)

    def to_latent_shape(self, x):
        (B, h, w, _) = x.shape
        (_, _, D) = self.latent_shape
        (rH, rW, _) = self.shape_divisor
        return x.reshape(B, h, w, rH, rW, D).permute(0, 1, 3, 2, 4, 5).reshape(B, h * rH, w * rW, D)

    def invalidate_codebook_cache(self):
        for cb in self.codebooks:
            cb.invalidate_codebook_cache()

    def forward(self, x):
        """(:273-281) -> (out = fl(x + fl(agg_d - x)), mean over depth of mean((x - agg_{i+1})^2), codes [B, h, w, d])"""
        if torch.is_grad_enabled() and x.requires_grad:
            return _RQFunction.apply(x, self, self.training)
        out, loss, codes, _ = _rq_forward(self, x, False, True, self.training)
        return out, loss, codes

    @torch.no_grad()
    def get_codes(self, x):
        """codes [B, h, w, d] alone (what RQVAE.get_codes takes from forward, rqvae.py:124-128): no loss, no gradient buffer"""
        return _rq_forward(self, x, False, False, self.training)[2]

    def _embed(self, code, mode, j, latent):
        if not isinstance(code, torch.Tensor) or not code.is_cuda:
            raise _lib.DvqError("code must be a tensor on the GPU: the dvq kernels run on the GPU only (no CPU fallback)")
        code = code.long().contiguous()
        B, h, w, depth = code.shape
        if latent:
            rH, rW, Dl = int(self.shape_divisor[0]), int(self.shape_divisor[1]), int(self.latent_shape[2])
        else:
            rH, rW, Dl = 1, 1, int(self.codebooks[0].weight.shape[1])
        D = rH * rW * Dl
        if depth > _lib.RQ_MAX_DEPTH:
            raise _lib.DvqError("RQBottleneck: depth %d above the kernels' limit %d" % (depth, _lib.RQ_MAX_DEPTH))
        books = _books(self, depth)
        ws = [cb.weight for cb in books]
        for t, wt in enumerate(ws):
            if not (wt.is_cuda and wt.dtype == torch.float32 and wt.is_contiguous()):
                raise _lib.DvqError("RQBottleneck: codebook %d must be a contiguous f32 tensor on the GPU" % t)
        if mode == _lib.RQ_EMBED_EACH:
            out = torch.empty((B, h * rH, w * rW, j + 1, Dl), dtype=torch.float32, device=code.device)
        else:
            out = torch.empty((B, h * rH, w * rW, Dl), dtype=torch.float32, device=code.device)
        if out.numel() == 0:
            return out
        ptrs = (ctypes.c_void_p * depth)(*[wt.data_ptr() for wt in ws])
        ks = (ctypes.c_int * depth)(*[wt.shape[0] for wt in ws])
        with _lib.on_device(code.device):
            checked.dvq_rq_embed_code_f32(ptrs, ks, depth, code.data_ptr(), B, h, w, rH, rW, Dl, D, mode, j,
                                          out.data_ptr(), _lib.stream_ptr(code.device))
        return out

    @torch.no_grad()
    def embed_code(self, code):
        """(:298-311) sum over depth of the codes' rows, fl(...fl(0 + e_0) + e_1 ...), in latent shape"""
        assert code.shape[1:] == self.code_shape
        return self._embed(code, _lib.RQ_EMBED_SUM, code.shape[-1] - 1, True)

    @torch.no_grad()
    def embed_code_with_depth(self, code, to_latent_shape=False):
        """(:314-334) the rows per depth, not summed: [B, h, w, d, D] (to_latent_shape: [B, H, W, d, Dl]), None"""
        assert code.shape[-1] == self.code_shape[-1]
        return self._embed(code, _lib.RQ_EMBED_EACH, code.shape[-1] - 1, bool(to_latent_shape)), None

    @torch.no_grad()
    def embed_partial_code(self, code, code_idx, decode_type='select'):
        """(:337-369) depth code_idx alone ('select') or the sum over depths 0 .. code_idx ('add'), in latent shape"""
        assert code.shape[1:] == self.code_shape
        assert code_idx < code.shape[-1]
        if decode_type == 'select':
            return self._embed(code, _lib.RQ_EMBED_SELECT, int(code_idx), True)
        if decode_type == 'add':
            return self._embed(code, _lib.RQ_EMBED_SUM, int(code_idx), True)
        raise NotImplementedError(f"{decode_type} is not implemented in partial decoding")

    @torch.no_grad()
    def get_soft_codes(self, x, temp=1.0, stochastic=False):
        """(:372-400) -> (softmax(-dist / temp) per depth [B, h, w, d, K], codes [B, h, w, d]).  Per depth one `soft_assign`
        on the residual (the assign's bit-exact distances, the softmax and the code in one kernel), then `dvq_rq_step_f32` with
        that depth's code.  Hard codes: the first-index argmin, equal to forward's (eval); stochastic: argmax of soft / q with
        q drawn per depth from torch's generator as torch.multinomial draws it, on the residual chain of the DRAWN codes, as
        the reference does it."""
        g = _RQGeom(self, x)
        soft = []

        def assign(i, cb, r):
            q = None
            if stochastic:
                q = torch.empty(g.N, cb.n_embed, dtype=torch.float32, device=r.device).exponential_(1)
            s, code, _ = soft_assign(r, cb.weight[:-1], cb._prep, temp, q)
            soft.append(s.reshape(g.B, g.h, g.w, 1, -1))
            return code

        codes = _rq_forward(self, x, False, False, False, assign=assign)[2]
        if not soft:                                  # empty batch
            return x.new_zeros((g.B, g.h, g.w, g.depth, self.codebooks[0].n_embed)), codes
        return torch.cat(soft, dim=-2), codes
