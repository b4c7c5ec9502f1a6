"""Test-side restatement of the decode head (codes -> the decoder's conv_in input) in numpy, plus the loaders of its golden
fixtures.  Imports no reference code.

  table64(E, W, b)      T = E W^T + b in float64 (W [C, D], b nullable)
  magnitude(E, W, b)    M = |E| |W|^T + |b|: what the conv's error bound is relative to
  head(T, F, L, codes)  fl(fl(T[codes] + F) + L) in float32 ops, NCHW; NaN rows for codes outside [0, rows)
"""
import json
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
EPS = 2.0 ** -24                                  # half an ulp of 1.0 in float32: one rounding


def crc(a):
    return int(zlib.crc32(np.ascontiguousarray(a).tobytes()))


def table64(E, W, b=None):
    T = E.astype(np.float64) @ W.astype(np.float64).reshape(W.shape[0], -1).T
    return T if b is None else T + b.astype(np.float64)[None, :]


def magnitude(E, W, b=None):
    M = np.abs(E.astype(np.float64)) @ np.abs(W.astype(np.float64).reshape(W.shape[0], -1)).T
    return M if b is None else M + np.abs(b.astype(np.float64))[None, :]


def head(T, F, L, codes):
    """T [rows, C] f32, F / L [C, H, W] f32 or None, codes [B, H, W] int -> [B, C, H, W] f32"""
    T = np.asarray(T, dtype=np.float32)
    rows = T.shape[0]
    codes = np.asarray(codes, dtype=np.int64)
    ok = (codes >= 0) & (codes < rows)
    h = T[np.where(ok, codes, 0)]                                        # [B, H, W, C]
    h = np.where(ok[..., None], h, np.float32(np.nan)).astype(np.float32)
    h = np.ascontiguousarray(np.moveaxis(h, 3, 1))
    if F is not None:
        h = (h + np.asarray(F, dtype=np.float32)[None]).astype(np.float32)
    if L is not None:
        h = (h + np.asarray(L, dtype=np.float32)[None]).astype(np.float32)
    return h


def gather_nchw(A, codes):
    """A [rows, C] -> A[codes] as [B, C, H, W] (codes in range)"""
    return np.moveaxis(A[np.asarray(codes, dtype=np.int64)], 3, 1)


def bound(M, T, F, L, codes, conv_rel):
    """conv_rel * M[code] + 4 * 2^-24 * (|T[code]| + |F| + |L|): the conv contract of include/dvq.h plus the four roundings
    of the two adds on both sides"""
    mag = np.abs(gather_nchw(T, codes)).astype(np.float64)
    for P in (F, L):
        if P is not None:
            mag = mag + np.abs(np.asarray(P, dtype=np.float64))[None]
    return conv_rel * gather_nchw(M, codes) + 4.0 * EPS * mag


def load(name):
    """a decode-head fixture as a dict; arrays too large for one file are stored as channel slabs in <name>_c<i>.npz parts
    (every committed file stays below 1 MiB) and concatenated here along the channel axis"""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    d["meta"] = json.loads(str(d["meta"]))
    nparts = int(d.get("parts", 0))
    if nparts:
        parts = [np.load(os.path.join(GOLDEN, "%s_c%d.npz" % (name, i))) for i in range(nparts)]
        for key, axis in (("pos_first", 0), ("pos_second", 0), ("h_in", 1)):
            if key in parts[0].files:
                d[key] = np.concatenate([p[key] for p in parts], axis=axis)
    return d


# ---- torch stand-ins with the attribute layout of the reference's decoder-side modules (restated, not imported) ----------
def stub_modules():
    """-> namespace of nn.Module classes: Fourier (coord + lff.ffm.conv + sin), Learned (row_embed / col_embed), Decoder
    (position_type dispatch as DecoderPositional.Decoder.forward, then conv_in; `h_in=` is the integrator's cut), FirstStage
    (quantize, post_quant_conv, decoder, get_code_emb_with_depth, decode) and Dualformer (decode_to_img, as
    dqtransformer_uncond_entropy.py:174-178)"""
    from types import SimpleNamespace

    import torch
    from torch import nn

    class _Con(nn.Module):
        def __init__(self, cin, cout):
            super().__init__()
            self.conv = nn.Conv2d(cin, cout, kernel_size=1)

        def forward(self, x):
            return self.conv(x)

    class _LFF(nn.Module):
        def __init__(self, hidden):
            super().__init__()
            self.ffm = _Con(2, hidden)

        def forward(self, x):
            return torch.sin(self.ffm(x))

    class Fourier(nn.Module):
        def __init__(self, coord_size, hidden_size):
            super().__init__()
            lin = torch.linspace(-1, 1, coord_size)
            xs = lin.view(1, 1, 1, -1).repeat(1, 1, coord_size, 1)
            ys = lin.view(1, 1, -1, 1).repeat(1, 1, 1, coord_size)
            self.coord = torch.cat((xs, ys), dim=1)
            self.lff = _LFF(hidden_size)

        def forward(self, x):
            return x + self.lff(self.coord.to(x.device))

    class Learned(nn.Module):
        def __init__(self, n_row, feats_dim):
            super().__init__()
            self.row_embed = nn.Embedding(n_row, feats_dim)
            self.col_embed = nn.Embedding(n_row, feats_dim)

        def forward(self, x):
            h, w = x.shape[-2:]
            x_emb = self.col_embed(torch.arange(w, device=x.device)).unsqueeze(0).repeat(h, 1, 1)
            y_emb = self.row_embed(torch.arange(h, device=x.device)).unsqueeze(1).repeat(1, w, 1)
            return x + (x_emb + y_emb).permute(2, 0, 1).unsqueeze(0).repeat(x.shape[0], 1, 1, 1)

    class Decoder(nn.Module):
        def __init__(self, in_ch, latent_size, position_type, block_in=8):
            super().__init__()
            self.conv_in = nn.Conv2d(in_ch, block_in, kernel_size=3, padding=1)
            self.position_type = position_type
            if position_type in ("learned", "learned-relative"):
                self.position_bias = Learned(latent_size, in_ch)
            elif position_type == "fourier":
                self.position_bias = Fourier(latent_size, in_ch)
            elif position_type == "fourier+learned":
                self.position_bias_fourier = Fourier(latent_size, in_ch)
                self.position_bias_learned = Learned(latent_size, in_ch)

        def position_block(self, h):
            if self.position_type in ("full", "fourier"):
                h = self.position_bias(h)
            elif self.position_type == "fourier+learned":
                h = self.position_bias_learned(self.position_bias_fourier(h))
            return h

        def forward(self, h, grain_indices, h_in=None):
            if h_in is None:
                h_in = self.position_block(h)
            return self.conv_in(h_in)

    class FirstStage(nn.Module):
        def __init__(self, quantize, post_quant_conv, decoder):
            super().__init__()
            self.quantize, self.post_quant_conv, self.decoder = quantize, post_quant_conv, decoder

        def get_code_emb_with_depth(self, code):
            return self.quantize.get_codebook_entry(code)

        def decode(self, quant, grain_indices=None):
            return self.decoder(self.post_quant_conv(quant), grain_indices)

    class Dualformer(nn.Module):
        def __init__(self, first_stage_model, permuter):
            super().__init__()
            self.first_stage_model, self.permuter = first_stage_model, permuter

        @torch.no_grad()
        def decode_to_img(self, coarse_content, fine_content, coarse_position, fine_position):
            idx = self.permuter.forward_back(coarse_content, fine_content, coarse_position, fine_position)
            quant = self.first_stage_model.get_code_emb_with_depth(idx)
            return self.first_stage_model.decode(quant.permute(0, 3, 1, 2))

    return SimpleNamespace(Fourier=Fourier, Learned=Learned, Decoder=Decoder, FirstStage=FirstStage, Dualformer=Dualformer)
