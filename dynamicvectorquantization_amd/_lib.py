"""ctypes binding of libdvq.so (include/dvq.h) -- the only bridge between the torch-facing
modules of this package and the HIP kernels.

There is NO fallback: if the shared library is missing or an entry point is absent the import
of this module raises.  torch is imported first so that libdvq.so binds to the HIP runtime torch
already loaded (same libamdhip64.so.7 SONAME) and can use torch's streams and device pointers.

The binding is derived from the header: at import `_parse_header` reads every `DVQ_API <ret> dvq_name(<args>);` declaration of
include/dvq.h and maps its C types to ctypes (`_CTYPES`; any pointer is c_void_p, `const char *` returned is c_char_p).  A type
outside that table, or a DVQ_API declaration that does not parse, raises: nothing defaults to int.  A new entry point needs its
declaration in the header and its definition in csrc/dvq_abi.hip, nothing here.  Two namespaces carry the same prototypes:
`lib.dvq_x(...)` returns the status code (tests, tools, bench), `checked.dvq_x(...)` raises DvqError on a non-zero one (the
package's own call sites).  The constants below restate the header's #defines; tests/test_abi_and_host.py pins them to it.
"""
import ctypes
import os
import re
import subprocess
import types

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# DVQ_LIBRARY: load another build of the same sources instead (tools/ use csrc/libdvq_tuning.so, made by
# `make -C csrc tuning`, which additionally exports dvq_tuning_buffers: in-kernel diagnostics and clock stamps)
LIB_PATH = os.environ.get("DVQ_LIBRARY") or os.path.join(CSRC, "libdvq.so")

DVQ_OK = 0
MODE_EXACT = 0
MODE_FILTER = 1
MODE_FILTER_PASS1 = 2   # profiling aid: only the dominant filter kernel
MODE_FILTER_WIDE = 3    # testing aid: force the two-blocks-per-wave pass-1 kernel (D = 256)
FILTER_MODES = (MODE_FILTER, MODE_FILTER_PASS1, MODE_FILTER_WIDE)
MODE_WS_CLEAN = 0x100   # flag OR-ed into a filter mode: the workspace is clean (include/dvq.h), no zeroing kernel is launched
GATE_F32 = 0
GATE_I64 = 1
GATE_ENTROPY = 2        # routed assign only: entropy map + threshold
RQ_MAX_DEPTH = 16       # DVQ_RQ_MAX_DEPTH: residual-quantization depth limit
RQ_EMBED_SUM, RQ_EMBED_SELECT, RQ_EMBED_EACH = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_RELU = 0, 1, 2
SAMPLE_MAX_V = 8192     # the sampling head's vocabulary limit (include/dvq.h: dvq_sample_head_f32)
TRANSFER_SAMPLED, TRANSFER_REMAIN = 0, 1
TRANSFER_SOS_NONE, TRANSFER_SOS_CONST, TRANSFER_SOS_COPY = 0, 1, 2
METRIC_L2, METRIC_DOT = 0, 1   # dvq_vq_score_assign_f32: s = -distance / s = dot product
DTYPE_F16, DTYPE_BF16 = 1, 2   # DVQ_DTYPE_*: the 16-bit latents of the *_x16 entry points
X16 = {torch.float16: DTYPE_F16, torch.bfloat16: DTYPE_BF16}
NHWC = 0x1000                  # DVQ_NHWC: channels_last branch features, OR-ed into the same argument as FEATURES(dtype)


def FEATURES(dtype):
    """DVQ_FEATURES(dtype) of include/dvq.h for a torch dtype: the flag OR-ed into `gate_dtype` of the route selects and `activation`
    of the router gate when the branch features are fp16 / bf16; 0 for float32"""
    return X16.get(dtype, 0) << 8


class DvqError(RuntimeError):
    pass


HEADER = os.path.join(os.path.dirname(_HERE), "include", "dvq.h")       # as csrc/Makefile finds it: ../../include/dvq.h
_CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
_DECL = re.compile(r"\s+([^();]+?)\s*\b(dvq_\w+)\s*\(([^()]*)\)\s*;")


def _ctype(text, name, is_param):
    """the ctypes type of one C parameter (`const float *z`, `int64_t N`) or return type; an unknown type raises -- no default"""
    if "*" in text:
        return ctypes.c_char_p if not is_param and text.split() == ["const", "char", "*"] else ctypes.c_void_p
    words = [w for w in text.split() if w != "const"]
    if is_param and len(words) > 1:
        words.pop()                                                      # the parameter's name
    if " ".join(words) not in _CTYPES:
        raise DvqError("include/dvq.h: %s: no ctypes type for `%s`" % (name, " ".join(text.split())))
    return _CTYPES[" ".join(words)]


def _parse_header(text):
    """{name: (restype, [argtypes])} of every `DVQ_API <ret> dvq_name(<args>);` declaration of the header text, in its order.
    Every use of DVQ_API other than its own #define has to parse as such a declaration."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+DVQ_API\b.*$", "", text, flags=re.M)
    protos = {}
    for chunk in re.split(r"\bDVQ_API\b", text)[1:]:
        m = _DECL.match(chunk)
        if m is None:
            raise DvqError("include/dvq.h: cannot parse the declaration `DVQ_API %s`" % " ".join(chunk.split(";")[0].split())[:160])
        ret, name, args = m.groups()
        args = [] if args.strip() in ("", "void") else args.split(",")
        protos[name] = (_ctype(ret, name, False), [_ctype(a, name, True) for a in args])
    return protos


def _read_header():
    if not os.path.exists(HEADER):
        raise DvqError("include/dvq.h not found at %s: the binding of libdvq.so is derived from it" % HEADER)
    with open(HEADER) as f:
        return _parse_header(f.read())


_PROTOTYPES = _read_header()
EXPORTS = tuple(_PROTOTYPES)


def build(force=False):
    """Compile csrc/*.hip for gfx950 with hipcc (csrc/Makefile) into csrc/libdvq.so."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


_VALUE_QUERIES = ("dvq_version", "dvq_vq_assign_narrow_tile_codes")   # return an int that is a value, not a status
# status calls whose refusals tests/golden/abi_rejections_det.json pins (tools/gen_golden_abi_rejections.py writes that table beside
# abi_rejections.json, which holds every other status call and is kept as it was): ordinary `int` status, checked.* raises as for the rest
_TABLED_APART = ("dvq_code_sums_det", "dvq_vq_backward_codebook_det_f32")
# GumbelQuantize's training step, added later still: tests/golden/abi_rejections_gumbel_train.json, written by the same tool
_TABLED_GUMBEL_TRAIN = ("dvq_vq_gumbel_forward_train_f32", "dvq_vq_gumbel_backward_f32")
# the int-returning entry points that tests/golden/abi_rejections.json does not cover: the value queries and the calls tabled apart
_INT_QUERIES = _VALUE_QUERIES + _TABLED_APART + _TABLED_GUMBEL_TRAIN


def _raise_on_error(rc, func, args):
    """errcheck of the checked entry points: what check(rc, name) raises"""
    if rc != DVQ_OK:
        raise DvqError("%s failed (rc=%d): %s" % (func.__name__, rc, lib.dvq_last_error_string().decode("utf-8", "replace")))
    return rc


def _load():
    if not os.path.exists(LIB_PATH):
        raise DvqError(
            "libdvq.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C %s` (hipcc --offload-arch=gfx950). There is no CPU fallback." % (LIB_PATH, CSRC))
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise DvqError("libdvq.so does not export %s (stale build?)" % name)
    protos = dict(_PROTOTYPES)
    if hasattr(lib, "dvq_tuning_buffers"):                 # tuning build only; not in the header
        protos["dvq_tuning_buffers"] = (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p])
    checked = types.SimpleNamespace()
    for name, (restype, argtypes) in protos.items():
        raw, fn = getattr(lib, name), lib[name]            # lib[name] is a function object of its own, lib.name the cached one
        raw.restype, raw.argtypes = restype, argtypes
        fn.restype, fn.argtypes = restype, argtypes
        if restype is ctypes.c_int and name not in _VALUE_QUERIES:
            fn.errcheck = _raise_on_error
        setattr(checked, name, fn)
    return lib, checked


# lib.dvq_x(...) returns the status code; checked.dvq_x(...) raises DvqError on a non-zero one (size queries: no difference)
lib, checked = _load()
# DVQ_MODE_WS_CLEAN exists since ABI 0.5.0 (an older build loaded through DVQ_LIBRARY for an A/B rejects the flag)
HAS_WS_CLEAN = lib.dvq_version() >= 500


def check(rc, what):
    if rc != DVQ_OK:
        msg = lib.dvq_last_error_string().decode("utf-8", "replace")
        raise DvqError("%s failed (rc=%d): %s" % (what, rc, msg))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)


def stream_ptr(device):
    """the current HIP stream of `device` as an integer (what the ABI takes as `void *stream`)"""
    if _raw_stream is not None and device.index is not None:
        return _raw_stream(device.index)                 # 0.2 us; torch.cuda.current_stream(..).cuda_stream builds a Stream object
    return torch.cuda.current_stream(device).cuda_stream


class _NoDeviceSwitch:
    def __enter__(self):
        return None

    def __exit__(self, *a):
        return False


_NO_SWITCH = _NoDeviceSwitch()


def on_device(device):
    """`with on_device(t.device):` -- torch.cuda.device(device) only when it is not the current device already (the context
    manager costs ~5 us per call: a fifth of a small op's host time, tools/module_overhead.py)"""
    if device.index is None or torch.cuda.current_device() == device.index:
        return _NO_SWITCH
    return torch.cuda.device(device)


def is_channels_last(t):
    """a 4-D [B, C, H, W] tensor in torch.channels_last memory format and NOT also contiguous (C = 1 or H = W = 1 satisfy both and
    stay NCHW): byte for byte the row-major matrix [B H W, C], which `channels_last_rows` views it as"""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last)


def channels_last_rows(t):
    """the [B H W, C] view of a channels_last tensor (no copy: the permuted tensor is contiguous)"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def rows_channels_last(rows, shape):
    """the inverse: rows [B H W, C] seen as the channels_last tensor of `shape` = (B, C, H, W)"""
    B, C, H, W = shape
    return rows.view(B, H, W, C).permute(0, 3, 1, 2)


def require_cuda_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise DvqError("%s is on %s: the dvq kernels run on the GPU only (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def require_cuda_latents(t, name, keep_channels_last=False):
    """require_cuda_f32 for LATENTS: float32, or float16 / bfloat16 (the *_x16 entry points of the dense assign, its backward
    and the EMA statistics); everything that is not a latent-shaped tensor stays with require_cuda_f32.
    keep_channels_last: a channels_last tensor (is_channels_last) comes back as it is, for the caller to serve as rows; every
    other layout that is not contiguous is copied as before."""
    if isinstance(t, torch.Tensor) and t.is_cuda and (t.dtype in X16 or t.dtype == torch.float32) and keep_channels_last \
            and is_channels_last(t):
        return t
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype in X16:
        return t if t.is_contiguous() else t.contiguous()
    if isinstance(t, torch.Tensor) and t.is_cuda and t.dtype != torch.float32:
        raise TypeError("%s must be float32, float16 or bfloat16, got %s" % (name, t.dtype))
    return require_cuda_f32(t, name)


def refuse_x16(t, name):
    """the ops that stay float32-only raise for 16-bit latents exactly what require_cuda_f32 raises (vq_assign itself takes them)"""
    if isinstance(t, torch.Tensor) and t.dtype in X16:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))


def ptr(t):
    return 0 if t is None else t.data_ptr()


from ._det import is_deterministic, set_deterministic, torch_deterministic  # noqa: E402,F401

DET_MAX_K = 16384              # DVQ_DET_MAX_K: the codebook size the fixed-order sums serve
DET_TILE, DET_RUN = 2048, 32   # DVQ_DET_TILE / DVQ_DET_RUN: the summation order's tile and run (include/dvq.h)


def det_workspace(B, D, HW, K, device):
    """a fresh workspace of the fixed-order sums (the caching allocator hands the same block back step after step)"""
    nbytes = checked.dvq_code_sums_det_workspace_bytes(B, D, HW, K)
    if nbytes == 0:
        raise DvqError("fixed-order sums: shape B=%d D=%d HW=%d K=%d unsupported (D %% 4 == 0, K <= %d)" % (B, D, HW, K, DET_MAX_K))
    return torch.empty(nbytes, dtype=torch.uint8, device=device)


def code_sums_into(z, codes, B, D, HW, K, counts, sums, deterministic=None):
    """counts [K] / sums [K, D] (float32, overwritten) of the GPU latents z -- [B, D, HW] contiguous, HW == 1: rows [N, D]; float32,
    float16 or bfloat16 -- under int64 `codes`: the statistics of the EMA update, k-means and the lucidrains codebooks.
    Switch off (`set_deterministic`): `dvq_ema_accumulate_nchw_f32` / `_x16`, float atomics, exactly as before the switch existed.
    Switch on: `dvq_code_sums_det`, one fixed summation order (a width that is no multiple of 4 runs with zero channels appended);
    K above DET_MAX_K: bincount and index_add_ under torch's own deterministic flag -- never the atomic kernel.  That fallback
    selects the valid tokens with a boolean mask, which synchronises with the host: it cannot be captured in a graph (the kernel
    path can), and it holds torch's process-wide flag on while it runs (`_det.torch_deterministic`: not thread-safe)."""
    x16 = X16.get(z.dtype, 0)
    st = stream_ptr(z.device)
    if not is_deterministic(deterministic):
        with on_device(z.device):
            if x16:
                checked.dvq_ema_accumulate_nchw_x16(z.data_ptr(), x16, codes.data_ptr(), B, D, HW, K, counts.data_ptr(), sums.data_ptr(), st)
            else:
                checked.dvq_ema_accumulate_nchw_f32(z.data_ptr(), codes.data_ptr(), B, D, HW, K, counts.data_ptr(), sums.data_ptr(), st)
        return
    sums = sums.view(K, D)
    if K > DET_MAX_K:
        rows = (z.reshape(B, D) if HW == 1 else z.reshape(B, D, HW).permute(0, 2, 1).reshape(-1, D)).to(torch.float32)
        flat = codes.reshape(-1)
        ok = (flat >= 0) & (flat < K)
        with torch_deterministic():
            counts.copy_(torch.bincount(flat[ok], minlength=K))
            sums.zero_().index_add_(0, flat[ok], rows[ok])
        return
    Dp, out = D, sums
    if D % 4 != 0:                                       # (the narrow width 3: a zero channel adds nothing to the other sums)
        Dp = (D + 3) // 4 * 4
        zp = torch.zeros((B, Dp, HW) if HW != 1 else (B, Dp), dtype=z.dtype, device=z.device)
        zp[:, :D] = z.reshape(B, D, HW) if HW != 1 else z.reshape(B, D)
        z, out = zp, torch.empty((K, Dp), dtype=torch.float32, device=z.device)
    ws = det_workspace(B, Dp, HW, K, z.device)
    with on_device(z.device):
        checked.dvq_code_sums_det(z.data_ptr(), x16, codes.data_ptr(), B, Dp, HW, K, counts.data_ptr(), out.data_ptr(),
                                  ws.data_ptr(), ws.numel(), st)
    if out is not sums:
        sums.copy_(out[:, :D])
