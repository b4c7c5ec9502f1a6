"""ctypes binding of libdvq.so (include/dvq.h) -- the only bridge between the torch-facing
modules of this package and the HIP kernels.

There is NO fallback: if the shared library is missing or an entry point is absent the import
of this module raises.  torch is imported first so that libdvq.so binds to the HIP runtime torch
already loaded (same libamdhip64.so.7 SONAME) and can use torch's streams and device pointers.
"""
import ctypes
import os
import subprocess

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

EXPORTS = (
    "dvq_version", "dvq_last_error_string", "dvq_codebook_prep_bytes", "dvq_codebook_prepare_f32",
    "dvq_vq_assign_workspace_bytes", "dvq_vq_assign_nchw_f32", "dvq_vq_assign_flat_f32", "dvq_vq_assign_fallback_count_offset",
    "dvq_embed_gather_f32",
    "dvq_vq_assign_routed_workspace_bytes", "dvq_vq_assign_routed_dual_f32", "dvq_vq_assign_routed_triple_f32",
    "dvq_vq_assign_routed_fallback_count_offset",
    "dvq_exchange_bytes", "dvq_exchange_pack", "dvq_exchange_unpack", "dvq_debug_filter_scores_f32",
    "dvq_qconv_prep_bytes", "dvq_qconv_prepare_f32", "dvq_qconv_f32", "dvq_qconv_select_f32",
    "dvq_vq_backward_nchw_f32", "dvq_vq_backward_codebook_nchw_f32", "dvq_vq_assign_qconv_f32", "dvq_vq_assign_routed_qconv_dual_f32", "dvq_vq_assign_routed_qconv_triple_f32",
    "dvq_fold_prep_bytes", "dvq_fold_prepare_f32", "dvq_vq_assign_fold_f32", "dvq_vq_assign_routed_fold_dual_f32",
    "dvq_vq_assign_routed_fold_triple_f32", "dvq_debug_fold_scores_f32",
    "dvq_entropy_gate_f32", "dvq_route_select_dual_f32", "dvq_route_select_dual_entropy_f32", "dvq_route_select_triple_f32",
    "dvq_entropy_map_f32", "dvq_ema_accumulate_nchw_f32", "dvq_restart_pick_i64", "dvq_ema_update_f32", "dvq_router_gate_workspace_bytes", "dvq_router_gate_prep_bytes", "dvq_router_gate_prepare_f32", "dvq_router_gate_prepare_norm_f32", "dvq_router_gate_f32", "dvq_permute_dual_count_i64", "dvq_permute_dual_forward_i64", "dvq_permute_dual_backward_i64",
    "dvq_route_train_workspace_bytes", "dvq_route_train_forward_f32", "dvq_route_train_backward_f32",
    "dvq_rq_workspace_bytes", "dvq_rq_residual_offset", "dvq_rq_step_f32", "dvq_rq_loss_f32", "dvq_rq_backward_f32",
    "dvq_rq_embed_code_f32",
    "dvq_sample_head_f32", "dvq_sample_transfer_count_i64", "dvq_sample_transfer_fill_i64",
    "dvq_decode_table_bytes", "dvq_decode_table_prepare_f32", "dvq_decode_head_f32",
    "dvq_vq_soft_assign_workspace_bytes", "dvq_vq_soft_assign_flat_f32",
    "dvq_vq_score_assign_f32", "dvq_vq_apply_codes_nchw_f32", "dvq_vq_apply_codes_flat_f32",
    "dvq_gumbel_prep_bytes", "dvq_gumbel_prepare_f32", "dvq_vq_gumbel_assign_workspace_bytes", "dvq_vq_gumbel_assign_f32",
    "dvq_vq_assign_narrow_workspace_bytes", "dvq_vq_assign_narrow_tile_codes", "dvq_vq_assign_narrow_nchw_f32",
    "dvq_vq_assign_narrow_flat_f32",
    "dvq_code_stats_f32", "dvq_code_stats_grain_f32",
    "dvq_vq_cdist_sample_assign_f32", "dvq_ortho_loss_workspace_bytes", "dvq_ortho_loss_forward_f32", "dvq_ortho_loss_backward_f32",
    "dvq_lucid_update_f32",
)


class DvqError(RuntimeError):
    pass


def build(force=False):
    """Compile csrc/*.hip for gfx950 with hipcc (csrc/Makefile) into csrc/libdvq.so."""
    args = ["make", "-C", CSRC, "-j8"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def _load():
    if not os.path.exists(LIB_PATH):
        raise DvqError(
            "libdvq.so not found at %s: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C %s` (hipcc --offload-arch=gfx950). There is no CPU fallback." % (LIB_PATH, CSRC))
    lib = ctypes.CDLL(LIB_PATH)
    for name in EXPORTS:
        if not hasattr(lib, name):
            raise DvqError("libdvq.so does not export %s (stale build?)" % name)
    vp, i32, i64, f32, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t
    lib.dvq_version.restype = i32
    lib.dvq_last_error_string.restype = ctypes.c_char_p
    lib.dvq_codebook_prep_bytes.restype = sz
    lib.dvq_codebook_prep_bytes.argtypes = [i32, i32]
    lib.dvq_codebook_prepare_f32.restype = i32
    lib.dvq_codebook_prepare_f32.argtypes = [vp, i32, i32, vp, sz, vp]
    lib.dvq_vq_assign_workspace_bytes.restype = sz
    lib.dvq_vq_assign_workspace_bytes.argtypes = [i32, i32, i32, i32, i32]
    lib.dvq_vq_assign_fallback_count_offset.restype = sz
    lib.dvq_vq_assign_fallback_count_offset.argtypes = [i32, i32, i32, i32]
    lib.dvq_vq_assign_nchw_f32.restype = i32
    lib.dvq_vq_assign_nchw_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, sz, i32, vp]
    lib.dvq_vq_assign_flat_f32.restype = i32
    lib.dvq_vq_assign_flat_f32.argtypes = [vp, vp, vp, vp, i64, i32, i32, f32, vp, vp, vp, vp, sz, i32, vp]
    lib.dvq_vq_assign_routed_workspace_bytes.restype = sz
    lib.dvq_vq_assign_routed_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, i32, i32]
    lib.dvq_vq_assign_routed_fallback_count_offset.restype = sz
    lib.dvq_vq_assign_routed_fallback_count_offset.argtypes = [i32, i32, i32, i32, i32, i32]
    lib.dvq_vq_assign_routed_dual_f32.restype = i32
    lib.dvq_vq_assign_routed_dual_f32.argtypes = [vp, i32, f32, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                                  vp, vp, vp, vp, vp, vp, vp, sz, i32, vp]
    lib.dvq_vq_assign_routed_triple_f32.restype = i32
    lib.dvq_vq_assign_routed_triple_f32.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                                    vp, vp, vp, vp, vp, vp, sz, i32, vp]
    lib.dvq_vq_backward_nchw_f32.restype = i32
    lib.dvq_vq_backward_nchw_f32.argtypes = [vp, vp, vp, vp, vp, vp, f32, i32, i32, i32, i32, vp, vp]
    lib.dvq_vq_backward_codebook_nchw_f32.restype = i32
    lib.dvq_vq_backward_codebook_nchw_f32.argtypes = [vp, vp, vp, vp, vp, f32, i32, i32, i32, i32, vp, vp]
    lib.dvq_vq_assign_qconv_f32.restype = i32
    lib.dvq_vq_assign_qconv_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, i32, vp, sz, i32, vp]
    lib.dvq_vq_assign_routed_qconv_dual_f32.restype = i32
    lib.dvq_vq_assign_routed_qconv_dual_f32.argtypes = [vp, i32, f32, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                                        vp, vp, vp, vp, vp, vp, vp, i32, vp, sz, i32, vp]
    lib.dvq_vq_assign_routed_qconv_triple_f32.restype = i32
    lib.dvq_vq_assign_routed_qconv_triple_f32.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32, f32,
                                                          vp, vp, vp, vp, vp, vp, i32, vp, sz, i32, vp]
    lib.dvq_fold_prep_bytes.restype = sz
    lib.dvq_fold_prep_bytes.argtypes = [i32, i32]
    lib.dvq_fold_prepare_f32.restype = i32
    lib.dvq_fold_prepare_f32.argtypes = [vp, i32, i32, vp, vp, vp, vp, sz, vp]
    lib.dvq_vq_assign_fold_f32.restype = i32
    lib.dvq_vq_assign_fold_f32.argtypes = [vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, sz, i32, vp]
    lib.dvq_vq_assign_routed_fold_dual_f32.restype = i32
    lib.dvq_vq_assign_routed_fold_dual_f32.argtypes = [vp, i32, f32, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32,
                                                       vp, vp, vp, vp, vp, vp, sz, i32, vp]
    lib.dvq_vq_assign_routed_fold_triple_f32.restype = i32
    lib.dvq_vq_assign_routed_fold_triple_f32.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, i32,
                                                         vp, vp, vp, vp, vp, sz, i32, vp]
    lib.dvq_debug_fold_scores_f32.restype = i32
    lib.dvq_debug_fold_scores_f32.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.dvq_qconv_prep_bytes.restype = sz
    lib.dvq_qconv_prep_bytes.argtypes = [i32]
    lib.dvq_qconv_prepare_f32.restype = i32
    lib.dvq_qconv_prepare_f32.argtypes = [vp, vp, i32, vp, sz, vp]
    lib.dvq_qconv_f32.restype = i32
    lib.dvq_qconv_f32.argtypes = [vp, vp, i32, i32, i32, vp, vp]
    lib.dvq_qconv_select_f32.restype = i32
    lib.dvq_qconv_select_f32.argtypes = [i32, vp, i32, f32, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    if hasattr(lib, "dvq_tuning_buffers"):                 # tuning build only
        lib.dvq_tuning_buffers.restype = i32
        lib.dvq_tuning_buffers.argtypes = [vp, vp]
    lib.dvq_debug_filter_scores_f32.restype = i32
    lib.dvq_debug_filter_scores_f32.argtypes = [vp, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    lib.dvq_exchange_bytes.restype = sz
    lib.dvq_exchange_bytes.argtypes = [i64, i64, i32, i32]
    lib.dvq_exchange_pack.restype = i32
    lib.dvq_exchange_pack.argtypes = [vp, vp, vp, ctypes.c_double, i32, i32, i64, i64, i32, vp, vp]
    lib.dvq_exchange_unpack.restype = i32
    lib.dvq_exchange_unpack.argtypes = [vp, i32, i32, i64, i64, i32, vp, vp, vp, vp]
    lib.dvq_embed_gather_f32.restype = i32
    lib.dvq_embed_gather_f32.argtypes = [vp, i32, i32, vp, i64, vp, vp]
    lib.dvq_entropy_gate_f32.restype = i32
    lib.dvq_entropy_gate_f32.argtypes = [vp, i64, f32, vp, vp]
    lib.dvq_route_select_dual_f32.restype = i32
    lib.dvq_route_select_dual_f32.argtypes = [vp, i32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.dvq_route_select_dual_entropy_f32.restype = i32
    lib.dvq_route_select_dual_entropy_f32.argtypes = [vp, f32, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.dvq_route_select_triple_f32.restype = i32
    lib.dvq_route_select_triple_f32.argtypes = [vp, i32, vp, vp, vp, i32, i32, i32, i32, vp, vp, vp, vp]
    lib.dvq_ema_accumulate_nchw_f32.restype = i32
    lib.dvq_ema_accumulate_nchw_f32.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, vp]
    lib.dvq_ema_update_f32.restype = i32
    lib.dvq_ema_update_f32.argtypes = [vp, vp, f32, f32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, i32, vp, vp]
    lib.dvq_restart_pick_i64.restype = i32
    lib.dvq_restart_pick_i64.argtypes = [ctypes.c_uint64, i64, i32, vp, vp]
    lib.dvq_router_gate_workspace_bytes.restype = sz
    lib.dvq_router_gate_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, i32, i32]
    lib.dvq_router_gate_prep_bytes.restype = sz
    lib.dvq_router_gate_prep_bytes.argtypes = [i32, i32, i32]
    lib.dvq_router_gate_prepare_f32.restype = i32
    lib.dvq_router_gate_prepare_f32.argtypes = [vp, i32, i32, i32, vp, sz, vp]
    lib.dvq_router_gate_prepare_norm_f32.restype = i32
    lib.dvq_router_gate_prepare_norm_f32.argtypes = [i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, sz, vp]
    lib.dvq_router_gate_f32.restype = i32
    lib.dvq_router_gate_f32.argtypes = [i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp,
                                        vp, vp, vp, vp, i32, i32, vp, vp, vp, sz, vp]
    lib.dvq_route_train_workspace_bytes.restype = sz
    lib.dvq_route_train_workspace_bytes.argtypes = [i32, i32, i32, i32, i32, i32, i32]
    _rt_in = [i32, vp, vp, vp, i32, i32, i32, i32, i32, f32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i32, i32, vp, f32]
    lib.dvq_route_train_forward_f32.restype = i32
    lib.dvq_route_train_forward_f32.argtypes = _rt_in + [vp, vp, vp, vp, vp, sz, vp]
    lib.dvq_route_train_backward_f32.restype = i32
    lib.dvq_route_train_backward_f32.argtypes = _rt_in + [vp, vp, vp, sz] + [vp] * 3 + [vp] * 6 + [vp] * 4 + [vp]
    lib.dvq_rq_workspace_bytes.restype = sz
    lib.dvq_rq_workspace_bytes.argtypes = [i64, i32, i32, i32]
    lib.dvq_rq_residual_offset.restype = sz
    lib.dvq_rq_residual_offset.argtypes = [i64, i32, i32, i32]
    lib.dvq_rq_step_f32.restype = i32
    lib.dvq_rq_step_f32.argtypes = [vp, vp, vp, i32, vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, sz, vp]
    lib.dvq_rq_loss_f32.restype = i32
    lib.dvq_rq_loss_f32.argtypes = [i64, i32, i32, vp, sz, vp, vp]
    lib.dvq_rq_backward_f32.restype = i32
    lib.dvq_rq_backward_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, i32, vp, sz, vp, vp]
    lib.dvq_rq_embed_code_f32.restype = i32
    lib.dvq_rq_embed_code_f32.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(i32), i32, vp, i32, i32, i32, i32, i32, i32, i32,
                                          i32, i32, vp, vp]
    lib.dvq_entropy_map_f32.restype = i32
    lib.dvq_entropy_map_f32.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    lib.dvq_permute_dual_count_i64.restype = i32
    lib.dvq_permute_dual_count_i64.argtypes = [vp, i32, i32, i32, vp, vp, vp]
    lib.dvq_permute_dual_forward_i64.restype = i32
    lib.dvq_permute_dual_forward_i64.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, ctypes.POINTER(i64),
                                                 vp, vp, vp, vp, vp, vp, vp]
    lib.dvq_permute_dual_backward_i64.restype = i32
    lib.dvq_permute_dual_backward_i64.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, i32, i64, i64, vp, vp]
    lib.dvq_sample_head_f32.restype = i32
    lib.dvq_sample_head_f32.argtypes = [vp, i64, i32, i32, f32, ctypes.POINTER(i64), vp, i64, i32, vp, i32, f32, i32, vp,
                                        vp, i64, vp, vp, vp]
    lib.dvq_sample_transfer_count_i64.restype = i32
    lib.dvq_sample_transfer_count_i64.argtypes = [vp, i64, i32, i32, i32, i64, i32, vp, vp, vp]
    lib.dvq_sample_transfer_fill_i64.restype = i32
    lib.dvq_sample_transfer_fill_i64.argtypes = [vp, i64, i32, i32, i32, i64, i32, i32, i32, i64, i64, i64, i32, vp, vp]
    lib.dvq_decode_table_bytes.restype = sz
    lib.dvq_decode_table_bytes.argtypes = [i32, i32]
    lib.dvq_decode_table_prepare_f32.restype = i32
    lib.dvq_decode_table_prepare_f32.argtypes = [vp, i32, i32, vp, vp, i32, vp, sz, vp]
    lib.dvq_decode_head_f32.restype = i32
    lib.dvq_decode_head_f32.argtypes = [vp, i32, i32, vp, i32, i32, vp, vp, vp, vp]
    lib.dvq_vq_soft_assign_workspace_bytes.restype = sz
    lib.dvq_vq_soft_assign_workspace_bytes.argtypes = [i64, i32, i32]
    lib.dvq_vq_soft_assign_flat_f32.restype = i32
    lib.dvq_vq_soft_assign_flat_f32.argtypes = [vp, vp, vp, i64, i32, i32, f32, vp, vp, vp, vp, vp, sz, vp]
    lib.dvq_vq_score_assign_f32.restype = i32
    lib.dvq_vq_score_assign_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, f32, vp, i64, vp, vp]
    lib.dvq_vq_apply_codes_nchw_f32.restype = i32
    lib.dvq_vq_apply_codes_nchw_f32.argtypes = [vp, vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, sz, vp]
    lib.dvq_vq_apply_codes_flat_f32.restype = i32
    lib.dvq_vq_apply_codes_flat_f32.argtypes = [vp, vp, vp, vp, i64, i32, i32, f32, vp, vp, vp, sz, vp]
    lib.dvq_gumbel_prep_bytes.restype = sz
    lib.dvq_gumbel_prep_bytes.argtypes = [i32, i32]
    lib.dvq_gumbel_prepare_f32.restype = i32
    lib.dvq_gumbel_prepare_f32.argtypes = [vp, vp, i32, i32, vp, sz, vp]
    lib.dvq_vq_gumbel_assign_workspace_bytes.restype = sz
    lib.dvq_vq_gumbel_assign_workspace_bytes.argtypes = [i32, i32]
    lib.dvq_vq_gumbel_assign_f32.restype = i32
    lib.dvq_vq_gumbel_assign_f32.argtypes = [vp, vp, vp, i32, i32, i32, i32, i32, f32, f32, vp, vp, vp, vp, vp, sz, vp]
    lib.dvq_vq_assign_narrow_workspace_bytes.restype = sz
    lib.dvq_vq_assign_narrow_workspace_bytes.argtypes = [i64]
    lib.dvq_vq_assign_narrow_tile_codes.restype = i32
    lib.dvq_vq_assign_narrow_tile_codes.argtypes = [i32]
    lib.dvq_vq_assign_narrow_nchw_f32.restype = i32
    lib.dvq_vq_assign_narrow_nchw_f32.argtypes = [vp, vp, vp, i32, i32, i32, i32, f32, vp, vp, vp, vp, sz, vp]
    lib.dvq_vq_assign_narrow_flat_f32.restype = i32
    lib.dvq_vq_assign_narrow_flat_f32.argtypes = [vp, vp, vp, i64, i32, i32, f32, vp, vp, vp, vp, sz, vp]
    lib.dvq_code_stats_f32.restype = i32
    lib.dvq_code_stats_f32.argtypes = [vp, i64, i32, vp, vp, vp, vp, vp]
    lib.dvq_code_stats_grain_f32.restype = i32
    lib.dvq_code_stats_grain_f32.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    lib.dvq_vq_cdist_sample_assign_f32.restype = i32
    lib.dvq_vq_cdist_sample_assign_f32.argtypes = [vp, vp, i32, i32, i32, i32, f32, vp, i64, vp, vp]
    lib.dvq_ortho_loss_workspace_bytes.restype = sz
    lib.dvq_ortho_loss_workspace_bytes.argtypes = [i32, i32, i32]
    lib.dvq_ortho_loss_forward_f32.restype = i32
    lib.dvq_ortho_loss_forward_f32.argtypes = [vp, i32, i32, i32, vp, vp, vp, sz, vp]
    lib.dvq_ortho_loss_backward_f32.restype = i32
    lib.dvq_ortho_loss_backward_f32.argtypes = [vp, vp, vp, i32, i32, i32, vp, vp, sz, vp]
    lib.dvq_lucid_update_f32.restype = i32
    lib.dvq_lucid_update_f32.argtypes = [i32, vp, vp, f32, f32, f32, i32, i32, vp, vp, vp, vp, vp, i32, i32, vp, vp]
    return lib


lib = _load()
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


def require_cuda_f32(t, name):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a torch.Tensor" % name)
    if not t.is_cuda:
        raise DvqError("%s is on %s: the dvq kernels run on the GPU only (no CPU fallback)" % (name, t.device))
    if t.dtype != torch.float32:
        raise TypeError("%s must be float32, got %s" % (name, t.dtype))
    return t if t.is_contiguous() else t.contiguous()


def ptr(t):
    return 0 if t is None else t.data_ptr()
