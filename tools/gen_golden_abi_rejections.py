#!/usr/bin/env python3
"""What the C ABI refuses, and in which words: tests/golden/abi_rejections.json.

  tools/gen_golden_abi_rejections.py [-o tests/golden/abi_rejections.json]
      calls the entry points of include/dvq.h with arguments that argument validation refuses and records, per call,
      {fn, args, rc, message}: the status code and the bytes of dvq_last_error_string().  Run it against a build of the commit
      whose behaviour is to be pinned (DVQ_LIBRARY=<path> selects another build than csrc/libdvq.so).
      The entry points of DET_FNS (dvq_code_sums_det, dvq_vq_backward_codebook_det_f32: ordinary status calls) have a table of their
      own, tests/golden/abi_rejections_det.json (--det-o), written in the same run: the first table is kept byte for byte as it was
      when they were added, and a later change that may touch it can merge the two.  GUMBEL_TRAIN_FNS (GumbelQuantize's training
      step) likewise: tests/golden/abi_rejections_gumbel_train.json (--gumbel-train-o).
  tools/gen_golden_abi_rejections.py --replay table.json
      makes the table's calls again and prints [[rc, message], ...] as JSON (tests/test_abi_rejections.py compares).

No call may get past validation: arguments are plain numbers, "pointers" are small integers (0 = null, 256 = aligned for every
check, 1 / 2 / 4 / 8 / 16 = misaligned for one of them) that nothing may dereference.  Both modes hide every GPU from the process
first, so a call that does get through fails at its launch (rc -4): recording refuses such a row -- take it out of the
ladders below -- and the replay shows it as a wrong rc.

A LADDER pins the order of an entry point's checks: its first call has an argument wrong for every check at once, so the first
check answers; each step repairs what that check looked at and the next check answers, down to the last one.

Neither torch nor the package is imported: the prototypes come from the header text, as in dynamicvectorquantization_amd/_lib.py.
"""
import argparse
import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dvq.h")
LIB = os.environ.get("DVQ_LIBRARY") or os.path.join(ROOT, "dynamicvectorquantization_amd", "csrc", "libdvq.so")
GOLDEN = os.path.join(ROOT, "tests", "golden", "abi_rejections.json")
GOLDEN_DET = os.path.join(ROOT, "tests", "golden", "abi_rejections_det.json")
DET_FNS = ("dvq_code_sums_det", "dvq_vq_backward_codebook_det_f32")     # their rows go to GOLDEN_DET
GOLDEN_GUMBEL_TRAIN = os.path.join(ROOT, "tests", "golden", "abi_rejections_gumbel_train.json")
GUMBEL_TRAIN_FNS = ("dvq_vq_gumbel_forward_train_f32", "dvq_vq_gumbel_backward_f32")     # and theirs to GOLDEN_GUMBEL_TRAIN
_CTYPES = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t}
REFUSALS = (-1, -2, -3)          # DVQ_EINVAL, DVQ_EUNSUPPORTED, DVQ_EWORKSPACE


def prototypes():
    """{name: [(parameter name, ctypes type)]} of the int-returning entry points of the header"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(HEADER).read(), flags=re.S)
    text = re.sub(r"^[ \t]*#[ \t]*define[ \t]+DVQ_API\b.*$", "", text, flags=re.M)
    protos = {}
    for chunk in re.split(r"\bDVQ_API\b", text)[1:]:
        ret, name, args = re.match(r"\s+([^();]+?)\s*\b(dvq_\w+)\s*\(([^()]*)\)\s*;", chunk).groups()
        if ret.strip() != "int" or args.strip() in ("", "void") or name == "dvq_vq_assign_narrow_tile_codes":    # (an int that is a value)
            continue
        params = []
        for a in args.split(","):
            words = [w for w in a.replace("*", " * ").split() if w != "const"]
            params.append((words[-1], ctypes.c_void_p if "*" in words else _CTYPES[" ".join(words[:-1])]))
        protos[name] = params
    return protos


def load():
    lib, protos = ctypes.CDLL(LIB), prototypes()
    lib.dvq_last_error_string.restype = ctypes.c_char_p
    for name, params in protos.items():
        getattr(lib, name).restype = ctypes.c_int
        getattr(lib, name).argtypes = [t for _, t in params]
    return lib, protos


def call(lib, fn, args):
    rc = getattr(lib, fn)(*args)
    return rc, lib.dvq_last_error_string().decode("utf-8")


# ---- the calls -------------------------------------------------------------------------------------------------------------
P = 256                  # a "pointer" that passes every null and alignment check
BIG = 1 << 30            # a byte count no size check refuses
ROWS = []                # (fn, {parameter: value})


def ladder(fn, first, *steps):
    """the first call and, per step, the call with that step's repairs added; what is not named: pointers P, numbers 1"""
    state = dict(first)
    ROWS.append((fn, dict(state)))
    for step in steps:
        state.update(step)
        ROWS.append((fn, dict(state)))


d = dict
WIDE = d(B=1 << 20, HW=1 << 12)       # 2^32 tokens: "tensor too large" wherever tokens are counted
ONE = d(B=1, HW=1)

ladder("dvq_codebook_prepare_f32", d(codebook=0, K=1024, D=100, prep=16, prep_bytes=16), d(codebook=P), d(D=256), d(prep_bytes=BIG))
ladder("dvq_codebook_prepare_f32", d(K=0))
ladder("dvq_fold_prepare_f32", d(codebook=0, K=1024, D=100, fold_prep=16, fold_prep_bytes=0), d(codebook=P), d(D=256),
       d(fold_prep_bytes=BIG), d(fold_prep=P, codebook_prep=16))
ladder("dvq_qconv_prepare_f32", d(weight=0, D=100, prep=16, prep_bytes=0), d(weight=P), d(D=128), d(prep_bytes=BIG))
ladder("dvq_gumbel_prepare_f32", d(weight=0, K=0, C=100, prep=16, prep_bytes=0), d(weight=P), d(K=64), d(C=64), d(prep_bytes=BIG),
       d(prep=P, bias=2))

# the dense assign, float32 and 16-bit latents
_assign = [d(z=0, B=0, D=100, mode=7, loss=P, ws=0, ws_bytes=0, K=64), d(z=P), WIDE, d(D=256), d(mode=1), ONE, d(ws=16), d(ws_bytes=BIG)]
ladder("dvq_vq_assign_nchw_f32", *_assign)
ladder("dvq_vq_assign_nchw_f32", d(D=64, K=64, mode=0, loss=0, ws=16, ws_bytes=0))          # no workspace needed: a misaligned one is refused all the same
ladder("dvq_vq_assign_nchw_f32", d(D=64, K=64, mode=0x101, loss=0, ws=P, ws_bytes=16))      # the clean-workspace flag over the filter mode
ladder("dvq_vq_assign_nchw_f32", d(D=64, K=64, mode=3, loss=0, ws=0, ws_bytes=BIG), d(mode=2))
ladder("dvq_vq_assign_nchw_x16", d(_assign[0], dtype=0, zq=1), d(dtype=3), d(dtype=2), d(z=P), d(zq=P), WIDE, d(D=256), d(mode=2),
       d(mode=0x103), d(mode=7), d(mode=1), ONE, d(ws=16), d(ws_bytes=BIG))
ladder("dvq_vq_assign_nchw_x16", d(dtype=1, z=2, zq=0, D=16, K=64, mode=0, loss=0, ws=16, ws_bytes=0), d(D=64))
ladder("dvq_vq_assign_flat_f32", d(N=0, z=0, D=100, mode=7, K=64), d(N=1 << 31), d(N=(1 << 31) - 1), d(z=P), d(D=128), d(mode=1, ws=0),
       d(ws=P, ws_bytes=16), d(ws=8, ws_bytes=BIG))

# its backward and the EMA statistics
_back = [d(z=0, g_zq=0, g_loss=0, B=0, D=100, codebook=8), d(z=P), d(g_loss=P), d(B=1), d(D=48)]
ladder("dvq_vq_backward_nchw_f32", *_back)
ladder("dvq_vq_backward_nchw_f32", d(D=0, g_loss=0), d(D=16, K=0), d(K=1, HW=0))
ladder("dvq_vq_backward_nchw_x16", d(_back[0], dtype=0), d(dtype=-1), d(dtype=1), d(z=1), d(g_loss=P), d(B=1), d(D=48), d(codebook=16),
       d(z=P, g_zq=1), d(g_zq=0, g_z=1))
ladder("dvq_ema_accumulate_nchw_f32", d(z=0, B=0), d(z=P), d(B=1, D=0), d(D=1, HW=0), d(HW=1, K=0))
ladder("dvq_ema_accumulate_nchw_f32", d(codes=0), d(codes=P, cluster_size=0), d(cluster_size=P, vectors_sum=0))
ladder("dvq_ema_accumulate_nchw_x16", d(dtype=0, z=0, B=0), d(dtype=3), d(dtype=2), d(z=1), d(z=2), d(B=1, K=0))

# the conv fused in, the conv folded in
ladder("dvq_vq_assign_qconv_f32", d(x=0, B=0, mode=0, qconv_prep=0, h_all=1, h_buf=0, D=128, K=1 << 20, ws=16, ws_bytes=0), d(x=P), WIDE,
       d(mode=1), d(qconv_prep=16), d(h_buf=P), d(D=256), d(qconv_prep=P, h_buf=2), d(h_buf=P), ONE, d(K=1024), d(ws_bytes=BIG))
ladder("dvq_vq_assign_qconv_f32", d(D=256, mode=2, K=64, ws=0, ws_bytes=BIG, h_all=0, h_buf=0))
ladder("dvq_vq_assign_fold_f32", d(x=0, B=0, D=100, qconv_prep=0, fold_prep=16, K=1 << 20, ws=16, ws_bytes=0, mode=0), d(x=P), WIDE, d(D=256),
       d(qconv_prep=P), d(fold_prep=P), ONE, d(K=1024), d(ws_bytes=BIG), d(ws=P))
ladder("dvq_vq_assign_fold_f32", d(D=64, K=64, mode=3, ws=0, ws_bytes=BIG))

# the routed assigns
_routed = [d(gate=0, B=0, gate_kind=5, D=100, hc=64, wc=64, mode=7, K=1 << 20, ws=16, ws_bytes=0), d(gate=P), d(B=40000), d(gate_kind=0),
           d(D=256), d(hc=4, wc=4), d(mode=1), d(B=1), d(K=1024), d(ws_bytes=BIG)]
ladder("dvq_vq_assign_routed_dual_f32", *_routed)
ladder("dvq_vq_assign_routed_dual_f32", d(D=256, K=64, hc=0), d(hc=1, wc=0), d(wc=1, K=0), d(K=64, mode=0, ws=0))
ladder("dvq_vq_assign_routed_triple_f32", d(_routed[0], h_median=0), d(h_median=P), d(gate=P), d(B=1), d(gate_kind=2), d(gate_kind=1), d(D=64),
       d(hc=32, wc=32), d(mode=2), d(K=1024, ws=0), d(ws=P, ws_bytes=16), d(ws=2, ws_bytes=BIG))
ladder("dvq_vq_assign_routed_qconv_dual_f32", d(D=256, K=64, mode=0, qconv_prep=0, ws=0), d(mode=1), d(qconv_prep=P, h_all=1, h_buf=0),
       d(D=128, h_buf=P), d(D=256))
ladder("dvq_vq_assign_routed_qconv_triple_f32", d(h_median=0, D=128, K=64, mode=1, ws=0), d(h_median=P), d(D=256, qconv_prep=1))
ladder("dvq_vq_assign_routed_fold_dual_f32", d(fold_prep=0, D=256, K=64, mode=0, ws=0), d(fold_prep=16), d(mode=1), d(fold_prep=P, qconv_prep=0))
ladder("dvq_vq_assign_routed_fold_triple_f32", d(h_median=0, fold_prep=0, D=256, K=64, mode=1, ws=0), d(h_median=P), d(fold_prep=P))

# soft, scored and sampled assigns, quantisation from given codes
ladder("dvq_vq_soft_assign_flat_f32", d(x=0, N=0, temp=0.0, D=100, K=1024, soft=0, ws=0, ws_bytes=5), d(x=2), d(N=1 << 31), d(N=1 << 30),
       d(temp=float("inf")), d(temp=1.0), d(D=256), d(N=1), d(x=P, prep=16), d(prep=P), d(ws=16, ws_bytes=0), d(ws_bytes=BIG))
ladder("dvq_vq_soft_assign_flat_f32", d(N=1, D=64, K=0))
_score = [d(x=0, B=0, metric=5, D=100, K=64, temp=0.0, u_numel=5), d(x=2), WIDE, d(metric=1), d(D=256), ONE, d(x=P, u=2), d(u=P, prep=16), d(prep=P),
          d(temp=1.0), d(u_numel=-64)]
ladder("dvq_vq_score_assign_f32", *_score)
ladder("dvq_vq_score_assign_f32", d(D=64, HW=1 << 20, B=1 << 10, K=1 << 11))               # N * K = 2^41
ladder("dvq_vq_cdist_sample_assign_f32", d(x=0, B=0, D=100, K=64, temp=0.0, u_numel=5, u=0), d(x=2, u=P), WIDE, d(D=256), ONE, d(x=P, u=2), d(u=P), d(temp=float("nan")), d(temp=0.5))
_apply = [d(z=0, B=0, D=100, K=64, zq=0, loss=0, ws=0, ws_bytes=7), d(z=2), WIDE, d(D=0), d(D=64), ONE, d(z=P, mask=2), d(mask=0, codebook=8),
          d(codebook=P, codes=4), d(codes=P), d(loss=P), d(ws=16, ws_bytes=0), d(ws_bytes=BIG)]
ladder("dvq_vq_apply_codes_nchw_f32", *_apply)
ladder("dvq_vq_apply_codes_flat_f32", d(N=0, z=0, D=100, K=64), d(N=1 << 31), d(N=5), d(z=P), d(D=32, K=0))

# GumbelQuantize, the narrow widths
ladder("dvq_vq_gumbel_assign_f32", d(z=0, B=0, C=100, K=64, d=0, tau=0.0, kl_K=0.0, ws=0, ws_bytes=9), d(z=2), d(B=1), d(d=8), WIDE, d(C=64), d(tau=0.5),
       d(kl_K=float("inf")), d(kl_K=64.0), ONE, d(z=P, codes=4), d(codes=P), d(ws=16, ws_bytes=0), d(ws_bytes=BIG))
ladder("dvq_vq_gumbel_assign_f32", d(C=64, K=64, d=8, q=0, tau=0.0, kl=0, ws=0, kl_K=-1.0))  # without q the temperature is not looked at
_narrow = [d(z=0, D=0, K=1 << 20, loss=P, ws=0, ws_bytes=9)]
ladder("dvq_vq_assign_narrow_nchw_f32", d(_narrow[0], B=0), d(z=4), WIDE, d(D=5), d(D=3), d(D=16), ONE, d(K=64, loss=2), d(loss=P, z=P, codebook=8),
       d(codebook=P), d(ws=16, ws_bytes=0), d(ws_bytes=BIG))
ladder("dvq_vq_assign_narrow_flat_f32", d(_narrow[0], N=0), d(z=4), d(N=1 << 31), d(K=0), d(K=1 << 20, D=64), d(D=8), d(N=7), d(K=64, codes=4),
       d(codes=P), d(z=P, zq=16 + 4), d(zq=16), d(zq=0), d(ws=8, ws_bytes=BIG))

# ---- one refusal at least for everything else that can refuse ---------------------------------------------------------------
ladder("dvq_embed_gather_f32", d(out=0, K=4, D=6), d(out=P, n=-1), d(n=1))
ladder("dvq_entropy_gate_f32", d(gate=0, n=-1), d(gate=P))
ladder("dvq_route_select_dual_f32", d(gate=0, gate_dtype=5, B=0), d(gate=P), d(gate_dtype=1))
ladder("dvq_route_select_dual_entropy_f32", d(entropy=0, wc=0), d(entropy=P))
ladder("dvq_route_select_triple_f32", d(h_median=0, cmask=0), d(cmask=P, C=0), d(C=8))
ladder("dvq_qconv_f32", d(h=0, B=0, D=100), d(h=P), WIDE, d(D=256))
ladder("dvq_qconv_select_f32", d(num_branches=4, gate=0, B=0, gate_kind=9, D=100, hc=1 << 15, wc=1 << 15), d(num_branches=3, h_median=0), d(h_median=P),
       d(gate=P), d(B=1), d(gate_kind=2), d(gate_kind=0), d(D=64))
ladder("dvq_debug_filter_scores_f32", d(xn=0, n=0, D=100), d(xn=P), d(n=1, K=64))
ladder("dvq_debug_fold_scores_f32", d(fold_prep=0, K=0, D=100), d(fold_prep=P), d(K=64))
ladder("dvq_vq_backward_codebook_nchw_f32", d(g_loss=0, D=0, K=8193), d(g_loss=P), d(D=64))
ladder("dvq_restart_pick_i64", d(out=0, n=15, k=1), d(out=P), d(n=1 << 32, k=2048), d(n=1 << 20, k=2049), d(k=0))
ladder("dvq_ema_update_f32", d(weight=0, K=0, cluster_size_out=P, restart=3, restart_rows=0, pick=0), d(weight=P), d(K=8), d(cluster_size_out=512),
       d(restart=1), d(restart=2))
ladder("dvq_code_stats_f32", d(codes=0, N=1, K=0), d(codes=P), d(K=1, N=-1), d(N=1, K=1 << 20))
ladder("dvq_code_stats_grain_f32", d(grain=0, G=4, K=1 << 20), d(grain=P), d(G=2, H=3, W=2), d(H=2))
ladder("dvq_router_gate_prepare_f32", d(num_branches=4, w1=0, C=100, hidden=32, w1_prep=16, w1_prep_bytes=16), d(num_branches=2), d(w1=P), d(C=648),
       d(C=256), d(w1_prep_bytes=BIG))
ladder("dvq_router_gate_prepare_norm_f32", d(num_branches=1, gn_w_median=0, C=256, hidden=32, w1_prep_bytes=16), d(num_branches=3), d(gn_w_median=P))
_gate = [d(num_branches=5, h_coarse=0, h_median=0, B=0, C=100, hc=16, wc=16, num_groups=7, activation=9, w1=0, hidden=0, gn_w_fine=0, ws=16, ws_bytes=16),
         d(num_branches=3), d(h_coarse=P), d(h_median=P), d(B=1), d(activation=1), d(w1=P, hidden=512), d(num_groups=25), d(gn_w_fine=P), d(C=1000),
         d(C=200, num_groups=200, hc=1, wc=1), d(num_groups=0), d(ws_bytes=BIG)]
ladder("dvq_router_gate_f32", *_gate)
ladder("dvq_route_train_forward_f32", d(_gate[0], tau=0.0, h_out=0), *_gate[1:6], d(activation=0, hidden=512), d(activation=1, w1=P), *_gate[7:9],
       d(tau=1.0), d(C=200, num_groups=0, wc=2048), d(wc=16), d(ws_bytes=BIG), d(ws=P))
ladder("dvq_route_train_backward_f32", d(_gate[0], tau=float("nan"), dw2=0, dgn_w_coarse=0), d(num_branches=2, h_coarse=P), d(h_median=0, B=1, activation=2),
       d(w1=P, hidden=1288), d(num_groups=25, gn_w_fine=P), d(tau=2.0), d(hidden=128, C=200), d(ws=P, ws_bytes=BIG), d(dw2=P))
ladder("dvq_rq_step_f32", d(ws=0, K=0, B=0, D=100, rH=2, rW=2, Dl=8, depth=0, i=-1, ws_bytes=0), d(ws=16), d(K=64), d(B=1), d(depth=17), d(depth=2),
       d(D=32, h=1 << 14, w=1 << 13), d(h=1, w=1), d(i=0), d(ws=P))
ladder("dvq_rq_step_f32", d(D=40, rH=1, rW=1, Dl=40, K=64, depth=1, i=0, ws_bytes=BIG))
ladder("dvq_rq_loss_f32", d(loss=0, N=0, D=100, depth=1, ws=16, ws_bytes=0), d(loss=P), d(N=1, depth=17), d(depth=1), d(D=32), d(ws=P))
ladder("dvq_rq_backward_f32", d(g_x=0, B=0, rH=2, rW=2, Dl=8, D=32, depth=1, ws=16, ws_bytes=0), d(g_x=P), d(B=1), d(ws=P))
ladder("dvq_rq_embed_code_f32", d(codebooks=0, rH=2, rW=2, Dl=8, D=33, depth=1), d(codebooks=P))
ladder("dvq_entropy_map_f32", d(out=0, B=0, H=250, W=256, patch=8), d(out=P), d(B=1), d(patch=16), d(B=1 << 22, H=256))
ladder("dvq_permute_dual_count_i64", d(maxes=0, B=0, hc=1 << 10, wc=1 << 10), d(maxes=P), d(B=1))
ladder("dvq_permute_dual_forward_i64", d(special=0, hc=0, order=2, Lc=0), d(special=P), d(hc=1), d(order=1))
ladder("dvq_permute_dual_backward_i64", d(target=0, wc=0, Lf=0), d(target=P), d(wc=1))
ladder("dvq_sample_head_f32", d(rules=0, B=0, V=1 << 20, temperature=0.0, top_k=-1, top_p=2.0, sample=1, q=0), d(rules=P), d(q=P, history_len=1, history=0),
       d(history_len=0), d(B=1), d(V=64), d(temperature=1.0), d(top_k=65), d(top_k=0))
_transfer = [d(coarse_position=0, B=0, Lc=4, hc=1 << 10, row_stride=3, variant=2), d(coarse_position=P), d(B=1), d(row_stride=4), d(hc=4), d(variant=1)]
ladder("dvq_sample_transfer_count_i64", d(_transfer[0], counts=0), *_transfer[1:])
ladder("dvq_sample_transfer_fill_i64", d(_transfer[0], out=0, order=2, sos_mode=3, L=0), *_transfer[1:], d(out=P), d(order=0), d(sos_mode=2))
ladder("dvq_decode_table_prepare_f32", d(codebook=0, rows=0, D=8, C=16, conv_weight=0, table=0, table_bytes=0), d(codebook=P), d(rows=4), d(C=8, conv_bias=P),
       d(conv_weight=P), d(table=8, D=1025), d(D=8, rows=1 << 30, C=1024), d(rows=4), d(table_bytes=BIG))
ladder("dvq_decode_head_f32", d(h_in=0, B=0, C=6, table=8), d(h_in=2), d(B=1), d(C=1028), d(C=8, B=1 << 16, HW=1 << 15), ONE, d(table=P))
ladder("dvq_exchange_pack", d(buf=0, b_local=2, b_max=1, grain_per_image=1, grain=0), d(buf=4), d(b_local=1), d(grain=P))
ladder("dvq_exchange_unpack", d(gathered=0, world=0, grain_per_image=1, grain=0), d(gathered=P), d(world=1))
# null codes and grain are an empty shard's alone (b_local = 0 gets past validation); the gathered buffer is read as doubles
ladder("dvq_exchange_pack", d(codes=0, b_local=1, grain_per_image=1, grain=0), d(codes=P))
ladder("dvq_exchange_unpack", d(gathered=4))
_ortho = [d(t=0, h=0, n=4, d=100, ws=0, ws_bytes=9), d(t=8), d(h=1), d(d=64, n=1 << 24), d(n=4)]
ladder("dvq_ortho_loss_forward_f32", *_ortho, d(t=P, loss=2), d(loss=P), d(ws=16, ws_bytes=0), d(ws_bytes=BIG))
ladder("dvq_ortho_loss_backward_f32", d(_ortho[0], grad=8), *_ortho[1:], d(t=P), d(grad=P), d(grad=512), d(ws=16, ws_bytes=0), d(ws_bytes=BIG))
ladder("dvq_lucid_update_f32", d(kind=2, counts=0, embed_avg=0, K=0, cluster_size_out=P, decay=2.0, embed=512, x=0), d(kind=0), d(counts=P), d(embed_avg=512),
       d(kind=1, sums=0), d(sums=P), d(K=8), d(cluster_size_out=1024), d(embed=1024), d(decay=0.5, threshold=-1.0), d(threshold=0.0))

# the direct form of the router gate keeps a 32-cell feature tile and the output-layer rows in LDS: what does not fit is refused in
# words (a triple router of C = 384 with the default hidden width, a dual single-layer router of C = 640, a small router with a very
# wide hidden layer), behind the group-size check and before the workspace's; the second ladder walks the checks of a dual router
_fits = d(num_groups=0, hc=4, wc=4, ws_bytes=BIG)
ladder("dvq_router_gate_f32", d(_fits, num_branches=3, C=384, activation=1, hidden=1152))
ladder("dvq_router_gate_f32", d(_fits, num_branches=2, h_median=0, C=640, activation=0, hidden=0))
ladder("dvq_router_gate_f32", d(_fits, num_branches=2, h_median=0, C=8, activation=1, hidden=16384))
ladder("dvq_router_gate_f32", d(num_branches=2, gate=0, h_median=P, wc=0, activation=-1, b1=0, hidden=16384, num_groups=-1, gn_b_coarse=0, C=12,
                                ws=0, ws_bytes=BIG), d(gate=P), d(h_median=0), d(wc=1), d(activation=2), d(b1=P), d(num_groups=3), d(gn_b_coarse=P),
       d(C=24, num_groups=12), d(num_groups=3), d(hidden=64), d(ws=16))

# the per-code sums in a fixed order: a table of their own (GOLDEN_DET)
ladder("dvq_code_sums_det", d(z=0, dtype=3, B=0, D=6, K=20000, HW=1 << 12, vectors_sum=8, ws=16, ws_bytes=0), d(z=1), d(dtype=2), d(B=1 << 20),
       d(D=4), d(K=64), ONE, d(z=2), d(vectors_sum=P), d(ws_bytes=BIG), d(ws=0))
ladder("dvq_code_sums_det", d(dtype=0, z=2, D=4, K=16385), d(K=16384), d(z=4, D=0), d(D=4, HW=0), d(HW=1, K=0), d(K=1, cluster_size=0))
ladder("dvq_vq_backward_codebook_det_f32", d(g_loss=0, B=0, D=6, K=20000, codebook=8, ws=16, ws_bytes=0), d(g_loss=P), d(B=1), d(D=8), d(K=8193),
       d(codebook=P), d(ws_bytes=BIG), d(ws=0), d(ws=P, g_weight=0))

# GumbelQuantize's training step: a table of their own (GOLDEN_GUMBEL_TRAIN).  The forward is the sweep's checked body: the same ladder,
# and the logits that may be neither null nor misaligned; the backward's checks in their order
ladder("dvq_vq_gumbel_forward_train_f32", d(z=0, B=0, C=100, K=64, d=0, tau=0.0, kl_K=0.0, ws=0, ws_bytes=9, logits=2), d(z=2), d(B=1), d(d=8), WIDE,
       d(C=64), d(tau=0.5), d(kl_K=float("inf")), d(kl_K=64.0), ONE, d(z=P), d(logits=P, codes=4), d(codes=P), d(ws=16, ws_bytes=0), d(ws_bytes=BIG))
ladder("dvq_vq_gumbel_forward_train_f32", d(C=64, K=64, d=8, logits=0))
ladder("dvq_vq_gumbel_backward_f32", d(logits=0, B=0, K=1 << 11, tau=0.0, kl_K=0.0, dlogits=2), d(logits=8), d(B=1 << 20, HW=1 << 12), d(tau=float("nan")),
       d(tau=2.0), d(kl_K=float("inf")), d(kl_K=8.0), d(B=1 << 10, HW=1 << 20), d(B=1, HW=1), d(dlogits=8), d(logits=P, dlogits=P, q=2),
       d(q=P, u=2), d(u=P, g_kl=1), d(g_kl=P))
ladder("dvq_vq_gumbel_backward_f32", d(logits=P, dlogits=512, q=512), d(q=P, HW=0), d(HW=1, dlogits=0))
# overlap is a matter of ranges (B HW K floats), not of equal pointers: logits, q, g_kl inside dlogits, u at an offset
_span = d(B=4, HW=4, K=4, logits=1 << 12, q=1 << 13, u=1 << 14, g_kl=1 << 15, dlogits=1 << 16)
ladder("dvq_vq_gumbel_backward_f32", d(_span, dlogits=(1 << 12) + 252), d(dlogits=(1 << 12) - 252), d(dlogits=(1 << 13) + 4), d(dlogits=(1 << 15) - 252),
       d(dlogits=(1 << 14) + 8), d(dlogits=(1 << 14) - 8))


def rows(protos):
    out = []
    for fn, named in ROWS:
        params = protos[fn]
        unknown = set(named) - {n for n, _ in params}
        assert not unknown, (fn, unknown)
        args = []
        for name, ctype in params:
            default = 0 if name == "stream" else P if ctype is ctypes.c_void_p else 1.0 if ctype in (ctypes.c_float, ctypes.c_double) else 1
            args.append(named.get(name, default))
        out.append({"fn": fn, "args": args})
    return out


def _num(v):
    """JSON has no inf / nan: the three are written as strings"""
    return {"inf": float("inf"), "-inf": float("-inf"), "nan": float("nan")}[v] if isinstance(v, str) else v


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("-o", default=GOLDEN)
    ap.add_argument("--det-o", default=GOLDEN_DET)
    ap.add_argument("--gumbel-train-o", default=GOLDEN_GUMBEL_TRAIN)
    ap.add_argument("--replay", metavar="TABLE")
    a = ap.parse_args()
    os.environ["HIP_VISIBLE_DEVICES"] = os.environ["ROCR_VISIBLE_DEVICES"] = ""      # before the library and the HIP runtime load
    lib, protos = load()
    if a.replay:
        table = json.load(open(a.replay))
        json.dump([call(lib, r["fn"], [_num(v) for v in r["args"]]) for r in table], sys.stdout)
        return
    table, seen = [], set()
    for r in rows(protos):
        rc, msg = call(lib, r["fn"], r["args"])
        if rc not in REFUSALS:
            sys.exit("%s%r got past validation (rc %d, %r): take the row out" % (r["fn"], tuple(r["args"]), rc, msg))
        r["args"] = [repr(v) if isinstance(v, float) and v - v != 0 else v for v in r["args"]]
        if json.dumps(r) not in seen:                         # a step that repeats the call before it
            seen.add(json.dumps(r))
            table.append(dict(r, rc=rc, message=msg))
    missing = set(protos) - {r["fn"] for r in table}
    assert not missing, "entry points without a row: %s" % sorted(missing)
    for path, part in ((a.o, [r for r in table if r["fn"] not in DET_FNS + GUMBEL_TRAIN_FNS]), (a.det_o, [r for r in table if r["fn"] in DET_FNS]),
                       (a.gumbel_train_o, [r for r in table if r["fn"] in GUMBEL_TRAIN_FNS])):
        with open(path, "w") as f:                            # a row per line
            f.write("[\n" + ",\n".join(json.dumps(r) for r in part) + "\n]\n")
        print("%d refusals of %d entry points -> %s" % (len(part), len({r["fn"] for r in part}), path))


if __name__ == "__main__":
    main()
