"""fp16 / bf16 branch features through the routing tail (DVQ_FEATURES of include/dvq.h): what the CPU and
the GPU tests share.

  * rounded(name, dtype): a row of tests/_gate_ref.CASES with its branches replaced by h.to(dtype).float() -- the values a 16-bit
    feature map holds, widened exactly -- and `logits64` recomputed on them.  The contract of the 16-bit gate is the float32 op on
    the widened values, so the float64 reference is taken on the widened values too.  Computed once per (row, dtype), read-only.
  * offset_view(t): the same values in a tensor that starts one element into its storage (2-byte aligned only for 16-bit types).
Nothing here calls the code under test."""
import copy
import functools

import torch

from tests import _gate_ref as G

DTYPES = [torch.float16, torch.bfloat16]
IDS = ["fp16", "bf16"]


@functools.lru_cache(maxsize=None)
def rounded(name, dtype):
    inp = copy.copy(G.case(name))
    inp.hs = [h.to(dtype).float() for h in inp.hs]
    inp.logits64 = G.reference64(inp)
    return inp


def offset_view(t):
    """t's values, contiguous, in a view that starts one element into a fresh storage"""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    return v
