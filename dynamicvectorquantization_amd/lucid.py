"""Drop-in for the reference's lucidrains-style quantizer (modules/vector_quantization/quantize_lucidrains.py): EuclideanCodebook,
CosineSimCodebook, VectorQuantize and orthogonal_loss_fn, on the HIP kernels of libdvq.so.

  target: dynamicvectorquantization_amd.lucid.VectorQuantize

Constructor arguments, defaults, buffer / parameter names and shapes (`_codebook.{initted [1], cluster_size [1, K], embed_avg
[1, K, D], embed [1, K, D]}`; no embed_avg in the cosine class; `embed` a Parameter iff orthogonal_reg_weight > 0) and return
structures are the reference's.  Inputs are f32 GPU tensors; anything else raises -- there is no torch fallback.

Dispatch of a forward:
  * Euclidean, sample_codebook_temp == 0: `vq_assign` in its default filter mode, codes only; eval: `embed_gather`; training:
    `apply_codes` (z + (e - z), the commitment loss) behind the parent package's given-codes autograd function;
  * Euclidean, temp > 0: N x K uniforms drawn as the reference draws them, then `dvq_vq_cdist_sample_assign_f32` -- the
    reference scores with -cdist (a square root), which does not commute with the Gumbel noise;
  * cosine: tokens and `embed` normalised as the reference does, `score_assign` on the dot product, the RAW rows gathered;
  * training: the code counts (`dvq_code_stats_f32`; cosine: counts and per-code sums of the normalised tokens,
    `dvq_ema_accumulate_nchw_f32`), ONE all_reduce of them when torch.distributed is initialised, then ONE kernel for the EMA of
    cluster_size, the new `embed` and code expiry (`dvq_lucid_update_f32`).  embed_avg is never written: the reference's embed_sum
    is dead code there, and `embed` = embed_avg / (smoothed cluster_size) is all its Euclidean update does;
  * the orthogonal regulariser and its gradient: `orthogonal_loss_fn`, two kernels, nothing of size n x n in memory.

Where the reference raises there is no behaviour to keep: use_cosine_sim = True builds the cosine codebook (the reference passes
it a `use_ddp` it does not take); `codebook` returns embed[0] (the reference reads an attribute that does not exist);
orthogonal_reg_active_codes_only raises NotImplementedError here; sync_codebook means "all_reduce iff torch.distributed is
initialised" (the reference calls all_reduce unconditionally and fails in a single process)."""
import math

import torch
import torch.distributed as dist
from torch import nn
from torch.nn import functional as F

from . import _lib
from ._prepared import InvalidatesPrepared
from .quantize import (KERNEL_WIDTHS, _CodebookPrep, _kmeans_lloyd, _batched_sample_vectors, _pad_channels, _restart_pick,
                       _vq_given_codes, _wide_width, embed_gather, score_assign, vq_assign)

checked = _lib.checked

__all__ = ["orthogonal_loss_fn", "EuclideanCodebook", "CosineSimCodebook", "VectorQuantize", "cdist_sample_assign"]


# ---- orthogonal regulariser ---------------------------------------------------------------------------------------------------
def _orthogonal_loss_torch(t):
    """the reference's expression (quantize_lucidrains.py:18-24)"""
    h, n = t.shape[:2]
    normed = F.normalize(t, p=2, dim=-1)
    identity = torch.eye(n, device=t.device).unsqueeze(0).expand(h, n, n)
    cosine_sim = torch.einsum('h i d, h j d -> h i j', normed, normed)
    return ((cosine_sim - identity) ** 2).sum() / (h * n ** 2)


class _OrthogonalLoss(torch.autograd.Function):
    """`dvq_ortho_loss_forward_f32` / `dvq_ortho_loss_backward_f32`: the Gram matrix of the normalised rows tiled over its upper
    triangle, squared and summed in the tiles' epilogues; backward = (4 g / (h n^2)) (C - I) C^ through F.normalize's backward,
    one sweep per block of rows.  The inverse norms of forward are kept for backward."""

    @staticmethod
    def forward(ctx, t):
        h, n, d = t.shape
        dev = t.device
        tc = t.detach().contiguous()
        rinv = torch.empty((h, n), dtype=torch.float32, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        ws = torch.empty(max(checked.dvq_ortho_loss_workspace_bytes(h, n, d), 256), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            checked.dvq_ortho_loss_forward_f32(tc.data_ptr(), h, n, d, rinv.data_ptr(), loss.data_ptr(),
                                               ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
        ctx.save_for_backward(tc, rinv)
        return loss

    @staticmethod
    def backward(ctx, g):
        tc, rinv = ctx.saved_tensors
        h, n, d = tc.shape
        dev = tc.device
        g = g.reshape(1).to(torch.float32).contiguous()
        grad = torch.empty_like(tc)
        ws = torch.empty(max(checked.dvq_ortho_loss_workspace_bytes(h, n, d), 256), dtype=torch.uint8, device=dev)
        with _lib.on_device(dev):
            checked.dvq_ortho_loss_backward_f32(tc.data_ptr(), rinv.data_ptr(), g.data_ptr(), h, n, d,
                                                grad.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream_ptr(dev))
        return grad


def orthogonal_loss_fn(t):
    """eq. (2) of arXiv 2112.00384: mean over h n^2 of (C - I)^2, C the cosines of the rows of t [h, n, d] ([n, d]: h = 1).
    f32 GPU tensors at the kernel widths d = 64 / 128 / 256: the fused kernels, differentiable, bit-reproducible run to run,
    nothing of size n x n allocated.  Anything else: the reference's torch expression."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("t must be [h, n, d] or [n, d], got %s" % (tuple(t.shape),))
    h, n, d = t.shape
    if (t.is_cuda and t.dtype == torch.float32 and d in KERNEL_WIDTHS and h >= 1 and n >= 1
            and checked.dvq_ortho_loss_workspace_bytes(h, n, d) != 0):
        return _OrthogonalLoss.apply(t)
    return _orthogonal_loss_torch(t)


# ---- the sampled assign against -cdist ----------------------------------------------------------------------------------------
def cdist_sample_assign(x, codebook, prep, temp, u):
    """x [B, D, *spatial] f32 cuda read in place (NCHW; [N, D]: row-major), codebook [K, D], u [N, K] uniforms, temp > 0 ->
    codes [B, *spatial] i64 = argmax(-cdist(x, codebook) / temp + gumbel(u)), one kernel (`dvq_vq_cdist_sample_assign_f32`):
    `score_assign` with the score -sqrt(max(d, 0)) of the assign's bit-exact distance d."""
    x = _lib.require_cuda_f32(x, "x")
    codebook = _lib.require_cuda_f32(codebook, "codebook")
    u = _lib.require_cuda_f32(u, "u")
    K, D = codebook.shape
    if x.dim() < 2 or x.shape[1] != D:
        raise ValueError("x must be [B, %d, ...] (channel dim %s != codebook dim %d)" % (D, tuple(x.shape[1:2]), D))
    temp = float(temp)
    if not (temp > 0.0 and math.isfinite(temp)):
        raise ValueError("temp must be finite and positive, got %r" % temp)
    B = x.shape[0]
    HW = 1
    for sdim in x.shape[2:]:
        HW *= sdim
    dev = x.device
    codes = torch.empty((B,) + tuple(x.shape[2:]), dtype=torch.int64, device=dev)
    if B * HW == 0:
        return codes
    Dp = _wide_width(D, "cdist_sample_assign")
    if Dp != D:
        x, codebook = _pad_channels(x, Dp), prep.padded_codebook(codebook, Dp)
    with _lib.on_device(dev):
        pbuf = prep.get(codebook)
        checked.dvq_vq_cdist_sample_assign_f32(
            x.data_ptr(), pbuf.data_ptr(), B, Dp, HW, K, temp, u.data_ptr(), u.numel(), codes.data_ptr(),
            _lib.stream_ptr(dev))
    return codes


def _draw_uniform(N, K, device):
    """the reference's noise draw (common_utils.py:27-29 on a [.., N, K] `dist`): the generator of `device` advances as there"""
    return torch.zeros(N, K, device=device).uniform_(0, 1)


def _ddp():
    return dist.is_available() and dist.is_initialized()


def _uniform_init(*shape):
    t = torch.empty(shape)
    nn.init.kaiming_uniform_(t)
    return t


# ---- the codebooks ------------------------------------------------------------------------------------------------------------
class _Codebook(InvalidatesPrepared, nn.Module):
    """What the two codebook classes share: buffers, layout handling, k-means initialisation, the training-step statistics and the
    update kernel.  `_tokens(x)` of the subclasses turns the module input into what the kernels read."""
    _prepared = ("_prep", "_prep_norm")
    _kind = 0                                    # dvq_lucid_update_f32: 0 Euclidean, 1 cosine

    def _setup(self, dim, codebook_size, kmeans_init, kmeans_iters, decay, eps, threshold_ema_dead_code, learnable_codebook,
               sample_codebook_temp, embed):
        self.decay = decay
        self.dim = dim
        self.codebook_size = codebook_size
        self.kmeans_iters = kmeans_iters
        self.eps = eps
        self.threshold_ema_dead_code = threshold_ema_dead_code
        self.sample_codebook_temp = sample_codebook_temp
        self.sample_fn = _batched_sample_vectors
        self.register_buffer('initted', torch.Tensor([not kmeans_init]))
        self.register_buffer('cluster_size', torch.zeros(1, codebook_size))
        if self._kind == 0:
            self.register_buffer('embed_avg', embed.clone())
        self.learnable_codebook = learnable_codebook
        if learnable_codebook:
            self.embed = nn.Parameter(embed)
        else:
            self.register_buffer('embed', embed)
        self._prep = _CodebookPrep()
        self._prep_norm = _CodebookPrep()        # of the L2-normalised embed (cosine)
        self._initted_host = not kmeans_init     # host mirror of `initted`: no device read per forward once it is set
        self._expire_pick = None                 # int64 GPU tensor: the tokens expired codes take, in order (tests inject it)
        self.assign_mode = _lib.MODE_FILTER

    def invalidate_codebook_cache(self):
        """call after writing `embed` through `.data` in eval mode"""
        self._prep.invalidate()
        self._prep_norm.invalidate()

    def _invalidate_prepared(self):
        super()._invalidate_prepared()
        self._initted_host = False

    # -- layouts: z is [B, D, *spatial] (channel-major, read in place) or [N, D] rows
    @staticmethod
    def _rows(z, channel_major):
        """token rows [N, D] in the reference's order ('b (h w) c'); a copy only for channel-major input"""
        if not channel_major:
            return z
        return z.reshape(z.shape[0], z.shape[1], -1).permute(0, 2, 1).reshape(-1, z.shape[1])

    def _check_world(self):
        if _ddp() and dist.get_world_size() > 1:
            raise NotImplementedError("k-means initialisation and code expiry across ranks (the reference's "
                                      "sample_vectors_distributed) are not implemented: run them with world size 1, or with "
                                      "kmeans_init=False and threshold_ema_dead_code=0")

    @torch.no_grad()
    def _init_embed(self, z, channel_major):
        if self._initted_host:
            return
        if bool(self.initted.item()):
            self._initted_host = True
            return
        self._check_world()
        flat = self._kmeans_tokens(self._rows(z.detach(), channel_major).contiguous())
        means = self.sample_fn(flat.unsqueeze(0), self.codebook_size)
        means, bins = _kmeans_lloyd(flat, means, self.kmeans_iters, cosine=self._kind == 1)
        self.embed.data.copy_(means)
        if self._kind == 0:
            self.embed_avg.data.copy_(means)
        self.cluster_size.data.copy_(bins)
        self.initted.data.copy_(torch.Tensor([True]))
        self._initted_host = True
        self.invalidate_codebook_cache()

    def _kmeans_tokens(self, rows):
        return rows

    def _picks(self, N, device):
        """[K] int64 token indices for expired codes.  N >= K: K distinct picks, no host read (the reference's randperm(N)[:num]
        for any num <= K).  N < K: the reference's own calls -- the number of expired codes read on the host, randperm when the
        batch has that many tokens, randint otherwise."""
        K = self.codebook_size
        if self._expire_pick is not None:
            pick = self._expire_pick.to(device=device, dtype=torch.int64).reshape(-1)
            if pick.numel() < K:
                pick = torch.cat([pick, pick.new_zeros(K - pick.numel())])
            return pick.contiguous()
        if N >= K:
            return _restart_pick(N, K, device).contiguous()
        return None

    @torch.no_grad()
    def _update(self, z, channel_major, codes, toks):
        """the training-mode tail of forward: statistics, one all_reduce, one update kernel"""
        K, D = self.codebook_size, self.dim
        dev = z.device
        N = codes.numel()
        codes = codes.reshape(-1)
        sums = None
        if self._kind == 0:
            cnt64 = torch.empty(K, dtype=torch.int64, device=dev)
            small = torch.empty(2, dtype=torch.int64, device=dev)
            perp = torch.empty((), dtype=torch.float32, device=dev)
            with _lib.on_device(dev):
                checked.dvq_code_stats_f32(codes.data_ptr(), N, K, cnt64.data_ptr(), small.data_ptr(), perp.data_ptr(),
                                           0, _lib.stream_ptr(dev))
            flat = counts = cnt64.to(torch.float32)
        else:
            flat = torch.empty(K * D + K, dtype=torch.float32, device=dev)
            sums, counts = flat[:K * D].view(K, D), flat[K * D:]
            _lib.code_sums_into(toks, codes, N, D, 1, K, counts, sums)
        if _ddp():
            dist.all_reduce(flat, op=dist.ReduceOp.SUM)            # the step's statistics: one collective
        thr = float(self.threshold_ema_dead_code)
        pick = None
        if thr > 0:
            self._check_world()
            pick = self._picks(N, dev)
        embed = self.embed.data[0]
        cs_new = torch.empty(K, dtype=torch.float32, device=dev)

        def launch(pick_t, threshold):
            B, HW = (z.shape[0], z[0, 0].numel()) if channel_major else (N, 1)
            with _lib.on_device(dev):
                checked.dvq_lucid_update_f32(
                    self._kind, counts.data_ptr(), _lib.ptr(sums), float(self.decay), float(self.eps), threshold, K, D,
                    self.cluster_size.data_ptr(), cs_new.data_ptr(), 0 if self._kind else self.embed_avg.data_ptr(), embed.data_ptr(),
                    z.data_ptr(), B, HW, _lib.ptr(pick_t), _lib.stream_ptr(dev))

        if thr > 0 and pick is None:
            # fewer tokens than codes: the reference's own calls, host read included (quantize_lucidrains.py:92, common_utils.py:43-50)
            launch(None, 0.0)
            expired = cs_new < thr
            num = int(expired.sum().item())
            if num:
                idx = torch.randperm(N, device=dev)[:num] if N >= num else torch.randint(0, N, (num,), device=dev)
                embed[expired] = F.normalize(self._rows(z.detach(), channel_major), p=2, dim=-1)[idx]
        else:
            launch(pick, thr if pick is not None else 0.0)
        self.cluster_size.data[0].copy_(cs_new)
        self.invalidate_codebook_cache()

    def forward(self, x):
        """x [..., D] channel-last, as the reference's codebooks take it -> (quantize [..., D] = the raw rows, embed_ind [...])"""
        x = _lib.require_cuda_f32(x, "x")
        z = x.reshape(-1, x.shape[-1])
        codes, toks = self._forward_codes(z, False)
        quantize = self._gather(codes.reshape(x.shape[:-1]))      # the rows as they were BEFORE this step's update
        self._train_step(z, False, codes, toks)
        return quantize, codes.reshape(x.shape[:-1])

    def _gather(self, codes):
        w = self.embed[0]
        if torch.is_grad_enabled() and w.requires_grad:
            return w[codes]                                       # (cold path: an autograd-visible gather)
        return embed_gather(w.detach(), codes)

    def _forward_codes(self, z, channel_major):
        """(codes [B, *spatial] / [N] of z, the normalised token rows or None); k-means initialisation on the first call"""
        D = self.dim
        _lib.require_cuda_f32(self.embed, "embed")
        if z.shape[1] != D:
            raise ValueError("channel dim %d != codebook dim %d" % (z.shape[1], D))
        _wide_width(D, type(self).__name__)
        self._init_embed(z, channel_major)
        if self.training:
            self.invalidate_codebook_cache()                      # the optimizer may have stepped `embed` through .data
        self._prep.track_users = self._prep_norm.track_users = self.training
        with torch.no_grad():
            return self._assign(z.detach(), channel_major)

    def _train_step(self, z, channel_major, codes, toks):
        """the codebook update, after the caller has gathered what it needs from the old rows"""
        if self.training:
            self._update(z.detach(), channel_major, codes, toks)


class EuclideanCodebook(_Codebook):
    """Reference quantize_lucidrains.py:28-149."""
    _kind = 0

    def __init__(self, dim, codebook_size, kmeans_init=False, kmeans_iters=10, decay=0.8, eps=1e-5, threshold_ema_dead_code=2,
                 learnable_codebook=False, sample_codebook_temp=0, use_ddp=False):
        super().__init__()
        embed = _uniform_init(1, codebook_size, dim) if not kmeans_init else torch.zeros(1, codebook_size, dim)
        self._setup(dim, codebook_size, kmeans_init, kmeans_iters, decay, eps, threshold_ema_dead_code, learnable_codebook,
                    sample_codebook_temp, embed)
        self.use_ddp = use_ddp

    def _assign(self, z, channel_major):
        w = self.embed.detach()[0]
        temp = float(self.sample_codebook_temp)
        if temp == 0.0:
            _, codes, _ = vq_assign(z, w, self._prep, want_zq=False, want_loss=False, mode=self.assign_mode)
        else:
            N = z.numel() // self.dim
            codes = cdist_sample_assign(z, w, self._prep, temp, _draw_uniform(N, self.codebook_size, z.device))
        if self._prep.track_users:
            self._prep.used(z.device)
        return codes, None


class CosineSimCodebook(_Codebook):
    """Reference quantize_lucidrains.py:151-284."""
    _kind = 1

    def __init__(self, dim, codebook_size, kmeans_init=False, kmeans_iters=10, decay=0.8, eps=1e-5, threshold_ema_dead_code=2,
                 learnable_codebook=False, sample_codebook_temp=0.):
        super().__init__()
        if not kmeans_init:
            embed = F.normalize(_uniform_init(1, codebook_size, dim), p=2, dim=-1)
        else:
            embed = torch.zeros(1, codebook_size, dim)
        self._setup(dim, codebook_size, kmeans_init, kmeans_iters, decay, eps, threshold_ema_dead_code, learnable_codebook,
                    sample_codebook_temp, embed)

    def _kmeans_tokens(self, rows):
        return F.normalize(rows, p=2, dim=-1)

    def _assign(self, z, channel_major):
        # rearrange first, then normalise along the last axis: the reference's calls on the reference's layout
        toks = F.normalize(self._rows(z, channel_major), p=2, dim=-1).contiguous()
        book = F.normalize(self.embed.detach()[0], p=2, dim=-1).contiguous()
        self._prep_norm.invalidate()
        temp = float(self.sample_codebook_temp)
        u = _draw_uniform(toks.shape[0], self.codebook_size, z.device) if temp > 0.0 else None
        codes = score_assign(toks, book, self._prep_norm, _lib.METRIC_DOT, temp, u)
        if self._prep_norm.track_users:
            self._prep_norm.used(z.device)
        if channel_major:
            codes = codes.reshape((z.shape[0],) + tuple(z.shape[2:]))
        return codes, toks


# ---- the main class -----------------------------------------------------------------------------------------------------------
class VectorQuantize(nn.Module):
    """Reference quantize_lucidrains.py:288-396.
      target: dynamicvectorquantization_amd.lucid.VectorQuantize"""

    def __init__(self, codebook_size, codebook_dim=None, decay=0.8, eps=1e-5, kmeans_init=False, kmeans_iters=10,
                 use_cosine_sim=False, threshold_ema_dead_code=0, channel_last=True, accept_image_fmap=False,
                 commitment_weight=1., orthogonal_reg_weight=0., orthogonal_reg_active_codes_only=False,
                 orthogonal_reg_max_codes=None, sample_codebook_temp=0., sync_codebook=True):
        super().__init__()
        if orthogonal_reg_active_codes_only:
            raise NotImplementedError("orthogonal_reg_active_codes_only: the reference indexes dim 0 of its [1, K, D] codebook with "
                                      "the active code ids and raises IndexError on the first training step; there is no "
                                      "behaviour to reproduce")
        self.eps = eps
        self.commitment_weight = commitment_weight
        has_codebook_orthogonal_loss = orthogonal_reg_weight > 0
        self.orthogonal_reg_weight = orthogonal_reg_weight
        self.orthogonal_reg_active_codes_only = orthogonal_reg_active_codes_only
        # accepted and inert, as in the reference: it compares the limit with codebook.shape[0], which is 1 (the head axis)
        self.orthogonal_reg_max_codes = orthogonal_reg_max_codes
        kw = dict(dim=codebook_dim, codebook_size=codebook_size, kmeans_init=kmeans_init, kmeans_iters=kmeans_iters, decay=decay,
                  eps=eps, threshold_ema_dead_code=threshold_ema_dead_code, learnable_codebook=has_codebook_orthogonal_loss,
                  sample_codebook_temp=sample_codebook_temp)
        if use_cosine_sim:
            self._codebook = CosineSimCodebook(**kw)
        else:
            self._codebook = EuclideanCodebook(use_ddp=sync_codebook, **kw)
        self.sync_codebook = sync_codebook       # collectives run iff torch.distributed is initialised
        self.accept_image_fmap = accept_image_fmap
        self.channel_last = channel_last

    @property
    def codebook(self):
        return self._codebook.embed[0]

    def forward(self, x):
        cb = self._codebook
        x = _lib.require_cuda_f32(x, "x")
        need_transpose = not self.channel_last and not self.accept_image_fmap
        if self.accept_image_fmap:
            if x.dim() != 4:
                raise ValueError("accept_image_fmap=True expects x [B, C, H, W]")
            z, channel_major = x, True                   # NCHW read in place by the kernels
        elif need_transpose:                             # [B, D, N]: already channel-major
            z, channel_major = x, True
        else:                                            # channel_last [B, ..., D] -> rows [N, D]
            z, channel_major = x.reshape(-1, x.shape[-1]), False
        codes, toks = cb._forward_codes(z, channel_major)
        w = cb.embed[0]
        if not self.training:
            q = cb._gather(codes.reshape(z.shape[0], -1) if channel_major else codes)
            quantize = q.permute(0, 2, 1).reshape(x.shape) if channel_major else q.reshape(x.shape)
            loss = torch.tensor([0.], device=x.device)
        else:
            zq, mean = _vq_given_codes(z, w.detach(), None, codes, cb._prep, cb.codebook_size, 1.0, 0.0)
            quantize = zq.reshape(x.shape)
            cb._train_step(z, channel_major, codes, toks)        # (the rows above are the ones from before the update)
            loss = torch.zeros(1, device=x.device)
            if self.commitment_weight > 0:
                loss = loss + mean * self.commitment_weight
            if self.orthogonal_reg_weight > 0:
                # on `embed` AFTER this step's update, h = 1, n = K, as the reference takes it
                loss = loss + orthogonal_loss_fn(cb.embed) * self.orthogonal_reg_weight
        if channel_major:
            embed_ind = codes
        else:
            embed_ind = codes.reshape(x.shape[:-1])
            if embed_ind.dim() > 2:                      # 'h ... d -> h (...) d' of a [B, ..., D] input
                embed_ind = embed_ind.reshape(x.shape[0], -1)
        return quantize, loss, (None, None, embed_ind)

    def get_codebook_entry(self, indices, *kwargs):
        indices = indices.view(indices.size(0), -1)
        return embed_gather(self._codebook.embed.detach()[0], indices)
