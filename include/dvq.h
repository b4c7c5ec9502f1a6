/*
 * dvq.h -- C ABI of libdvq.so: the MI355X (gfx950) implementation of the DQ-VAE
 * vector-quantization hot path.
 *
 * The reference (Corleone-Huang/DynamicVectorQuantization) is pure Python and
 * has no FFI of its own; each entry point below replaces the listed PyTorch op
 * sequence of the reference, and is what a ctypes binding in the reference
 * would call (INTEGRATION.md shows the stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch
 *     tensor's data_ptr()); nothing is allocated or freed inside;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); calls
 *     are stream-ordered, never synchronise, and are re-entrant: the library keeps
 *     no mutable process-wide state and reads no environment variable (kernel
 *     choices are compile-time constants; the A/B switches of the tuning build,
 *     libdvq_tuning.so made by `make tuning`, are not part of this ABI);
 *   - return value: DVQ_OK (0) or a negative DVQ_E* code; the message of the
 *     last failure on the calling thread is dvq_last_error_string();
 *   - tensors are dense, C-contiguous, float32 unless stated; code indices and
 *     grain indices are int64 (the reference's dtype);
 *   - channel counts (codebook_dim D): the assign kernels are instantiated for 64, 128 and
 *     256 (every reference config uses 256); other values return DVQ_EUNSUPPORTED.  A
 *     multiple of 32 below 256 (32, 96, 160, 192, 224) is served EXACTLY at the next kernel
 *     width by appending zero channels to latents and codebook -- a zero channel adds
 *     fma(0, 0, acc) = acc to the dot chain and + 0 to the norm's partial sums, whose 32-way
 *     grouping does not depend on D -- which is what the Python drop-in does
 *     (quantize.py: _padded_width); divide the returned loss mean by D / D_padded.
 *     The NARROW widths 4, 8 and 16 (and 3, as 4 with one zero channel) have entry points of their own,
 *     dvq_vq_assign_narrow_*_f32 below; every other entry point refuses them as before.
 *
 * Versions (dvq_version() = 100 major + minor; re-query every *_bytes function after an upgrade: buffer sizes are part of a version)
 *   0.20.0 DVQ_NHWC: the same three entry points take channels_last branch features ([B, rows, cols, C]: a torch.channels_last tensor's
 *          bytes) when DVQ_NHWC is OR-ed into the same enumerated argument, alone or with DVQ_FEATURES(dtype); h_out of the selects is
 *          then channels_last too.  The dtype field is bits 8 - 11 of the argument, the layout bit 12, any bit above it DVQ_EINVAL.
 *          Workspace and prep sizes are unchanged; without the flag nothing changed; no new entry point.
 *          Added later under the same version number (detect them by their symbols): dvq_code_sums_det, dvq_vq_backward_codebook_det_f32
 *          and their *_workspace_bytes queries -- the per-code sums of the training step (EMA statistics, codebook gradient) in one
 *          documented, fixed summation order, without float atomics.  Nothing else changed.
 *          Added later still, also under 0.20.0: dvq_vq_gumbel_forward_train_f32 and dvq_vq_gumbel_backward_f32 -- GumbelQuantize's training
 *          step in its hard form: the sweep of dvq_vq_gumbel_assign_f32 that also writes the logits, and the streaming kernel that turns
 *          them, the variates and embed . dL/dz_q into dL/dlogits.  Nothing else changed.
 *   0.19.0 DVQ_FEATURES(dtype): dvq_route_select_dual_f32, dvq_route_select_triple_f32 and dvq_router_gate_f32 take fp16 / bf16 branch
 *          features when DVQ_FEATURES(DVQ_DTYPE_F16 / DVQ_DTYPE_BF16) is OR-ed into their enumerated argument (gate_dtype, activation);
 *          the h_* / h_out parameters of the three are declared `const void *` / `void *` for that (binary- and source-compatible
 *          for C callers).  Without the flag nothing changed; no new entry point.
 *   0.18.0 Row-major latents [N, D] -- token rows, or a channels_last (NHWC) image map, which is the same bytes -- on the training side:
 *          dvq_vq_backward_nchw_f32 / _x16, dvq_vq_backward_codebook_nchw_f32 and dvq_ema_accumulate_nchw_f32 / _x16 called with B = N,
 *          HW = 1 run kernels whose accesses follow the rows (the backward: where z, g_zq and g_z are 16-byte aligned; same bits as
 *          before).  With HW = 1 dvq_ema_accumulate_nchw_* combines equal codes of a tile for every K.  No signature, status or message changed.
 *   0.17.1 dvq_router_gate_f32 refuses (DVQ_EUNSUPPORTED, naming the bytes) a shape whose 32-cell feature tile and output-layer rows do not
 *          fit one workgroup's LDS -- until now it failed in the launch with a bare HIP status -- and dvq_router_gate_workspace_bytes
 *          returns 0 for it; a dual router of C = 96 or 384 behind GroupNorm groups of whole octets of channels, until now a launch
 *          failure as well, is served.  Nothing else changed.
 *   0.17.0 DVQ_DTYPE_F16 / DVQ_DTYPE_BF16, dvq_vq_assign_nchw_x16, dvq_vq_backward_nchw_x16, dvq_ema_accumulate_nchw_x16 (new): the dense
 *          assign, its backward and the EMA statistics on fp16 / bf16 latents (an encoder run under autocast), everything else float32.
 *          Nothing else changed.
 *   0.16.0 dvq_vq_cdist_sample_assign_f32, dvq_ortho_loss_workspace_bytes, dvq_ortho_loss_forward_f32, dvq_ortho_loss_backward_f32,
 *          dvq_lucid_update_f32 (new): the lucidrains-style codebooks (quantize_lucidrains.py) -- the sampled assign against -cdist, the
 *          orthogonal regulariser with its gradient, and the per-step codebook update with code expiry.  Nothing else changed.
 *   0.15.0 dvq_code_stats_f32, dvq_code_stats_grain_f32 (new): code histogram, codes in use, perplexity and the optional one-hot matrix of
 *          a batch of codes -- what VectorQuantizer / EMAVectorQuantizer return besides z_q -- and the same per grain.  Nothing else changed.
 *   0.14.0 dvq_vq_assign_narrow_workspace_bytes, dvq_vq_assign_narrow_tile_codes, dvq_vq_assign_narrow_nchw_f32,
 *          dvq_vq_assign_narrow_flat_f32 (new): the exact assign at the narrow widths D = 4, 8, 16 (3 by one zero channel).  Nothing else changed.
 *   0.13.0 dvq_gumbel_prep_bytes, dvq_gumbel_prepare_f32, dvq_vq_gumbel_assign_workspace_bytes, dvq_vq_gumbel_assign_f32 (new): GumbelQuantize's
 *          hard forward -- projection, Gumbel argmax, KL term and z_q -- as one sweep.  Nothing else changed.
 *   0.12.0 dvq_vq_score_assign_f32, dvq_vq_apply_codes_nchw_f32, dvq_vq_apply_codes_flat_f32 (new), DVQ_METRIC_L2 / DVQ_METRIC_DOT: the
 *          scored / temperature-sampled assign of MaskVectorQuantize / VectorQuantize and quantisation from given codes.  Nothing else changed.
 *   0.11.0 dvq_vq_soft_assign_workspace_bytes, dvq_vq_soft_assign_flat_f32 (new): get_soft_codes as one kernel -- the assign's
 *          bit-exact distances, softmax(-d / temp), the hard code or the multinomial draw.  Nothing else changed.
 *   0.10.0 dvq_decode_table_bytes, dvq_decode_table_prepare_f32, dvq_decode_head_f32 (new): codes -> the input of the decoder's
 *          conv_in (codebook gather, post_quant_conv and the decoder's position biases as one kernel).  Nothing else changed.
 *   0.9.0  dvq_sample_head_f32, dvq_sample_transfer_count_i64, dvq_sample_transfer_fill_i64 (new): the sampling step and the
 *          coarse -> fine position transfer of stage-2 generation.  top_k = 0 and top_p = 0 switch the filter off (the reference's
 *          None); any other k < 1 or p outside (0, 1] is DVQ_EINVAL.  Nothing else changed.
 *   0.8.0  dvq_rq_workspace_bytes, dvq_rq_residual_offset, dvq_rq_step_f32, dvq_rq_loss_f32, dvq_rq_backward_f32,
 *          dvq_rq_embed_code_f32 (new): residual quantization (RQBottleneck) around the flat assign.  Nothing else changed.
 *   0.7.0  dvq_route_train_workspace_bytes, dvq_route_train_forward_f32, dvq_route_train_backward_f32 (new): the training-mode
 *          routing tail (feature-router gate, gumbel-hard select, gate_grad scale) and its backward.  Nothing else changed.
 *   0.6.0  dvq_ema_update_f32 (new); the conv-fused assigns (dvq_vq_assign_qconv_f32, dvq_vq_assign_routed_qconv_*_f32) take h_buf = NULL: no scratch tensor
 *          (0.3 - 0.5 required a full-size one); dvq_entropy_map_f32 refuses more than 2^30 patches per call; DVQ_MODE_WS_CLEAN's
 *          contract spelled out (valid for the same entry point and shape only).  No signature changed.
 *   0.5.0  DVQ_MODE_WS_CLEAN (self-cleaning workspace), dvq_vq_assign_flat_f32, dvq_restart_pick_i64,
 *          dvq_router_gate_prepare_norm_f32; DVQ_COUNTER_BYTES, the filter workspace (+ split buffer) and the gate's weight
 *          prep (+ 256-byte tail) grew: buffers sized by a 0.4.x build are too small for 0.5 and later.
 */
#ifndef DVQ_H_
#define DVQ_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* libdvq.so is built with -fvisibility=hidden: the entry points below are its whole dynamic symbol table */
#define DVQ_API __attribute__((visibility("default")))

#define DVQ_OK            0
#define DVQ_EINVAL       (-1)  /* bad argument (null pointer, non-positive size, ...) */
#define DVQ_EUNSUPPORTED (-2)  /* shape outside what the kernels implement            */
#define DVQ_EWORKSPACE   (-3)  /* workspace / prep buffer too small                   */
#define DVQ_EHIP         (-4)  /* HIP runtime error on launch                         */

/* assign modes */
#define DVQ_MODE_EXACT   0  /* every (token, code) distance by the exact fp32 MFMA chain     */
#define DVQ_MODE_FILTER  1  /* fp16-MFMA filter with a rigorous error bound; every token that  */
                            /* is not provably decided is re-evaluated by the exact chain.     */
                            /* Output is identical to DVQ_MODE_EXACT.                          */
#define DVQ_MODE_FILTER_PASS1 2  /* profiling aid: ONLY the pass-1 (fp16 filter) kernel of DVQ_MODE_FILTER, */
                                 /* the dominant kernel; queued tokens keep their provisional code, the     */
                                 /* loss is not finalised.  Not a production mode.                          */
#define DVQ_MODE_FILTER_WIDE 3   /* testing aid: DVQ_MODE_FILTER with the two-blocks-per-wave pass-1 kernel */
                                 /* forced (D = 256); normally chosen automatically for K >= 2048 and       */
                                 /* >= 131072 tokens.  Same output.                                         */

/* Flag, OR-ed into `mode` of the filter-path ops (every dvq_vq_assign_* entry point; ignored in DVQ_MODE_EXACT): the caller
 * guarantees that this workspace is CLEAN FOR THIS CALL'S LAYOUT and that no other stream is using it.  Clean means one of:
 *   (a) the whole workspace was zero-filled (hipMemsetAsync / torch.zeros over all of its bytes) and no op has used it since, or
 *   (b) the last call that used it was a filter-path op WITHOUT DVQ_MODE_FILTER_PASS1 that returned DVQ_OK, through an entry
 *       point of the SAME WORKSPACE LAYOUT and with the SAME shape arguments (B, D, HW or hc / wc, K) as this call.  The entry
 *       points of one group place the live words by one layout function and may hand a clean workspace to each other:
 *         dense   dvq_vq_assign_nchw_f32, dvq_vq_assign_qconv_f32, dvq_vq_assign_fold_f32, and dvq_vq_assign_flat_f32 as the
 *                 dense op with B = N, HW = 1   (dvq_vq_assign_workspace_bytes)
 *         dual    dvq_vq_assign_routed_dual_f32, _routed_qconv_dual_f32, _routed_fold_dual_f32
 *         triple  dvq_vq_assign_routed_triple_f32, _routed_qconv_triple_f32, _routed_fold_triple_f32
 *                 (dvq_vq_assign_routed_workspace_bytes with num_branches = 2 / 3)
 * (b) is shape-bound because the live words -- the 1-KiB counter block and the resolver's chunk tickets -- sit BEHIND the loss
 * partials, whose size is a function of B * HW, and the number of tickets is a function of the queue capacity (also B * HW): an
 * op leaves exactly ITS live words zero (its last consumer workgroup puts every counter back), not those of another shape's
 * layout.  A workspace that is merely large enough but was last used with other shape arguments is NOT clean: passing the flag
 * then lets pass 1 index its lists with stale counters (out-of-bounds device writes).  Keep one workspace per (stream, layout
 * group, shape) -- what the Python classes do, quantize._CodebookPrep.workspace -- or drop the flag when the shape changes.
 * With the flag no zeroing kernel is launched: one kernel boundary (~5 us) less per op.  Without it the op zeroes what it needs
 * first and any bytes are fine (the behaviour of versions before 0.5.0). */
#define DVQ_MODE_WS_CLEAN 0x100

/* gate kinds for the router select / routed assign */
#define DVQ_GATE_F32 0      /* float32 gate logits [.., G]                                      */
#define DVQ_GATE_I64 1      /* int64 gate [.., G] (what DualGrainFixedEntropyRouter returns)    */
#define DVQ_GATE_ENTROPY 2  /* routed assign only: float32 entropy map [B, hc, wc] + threshold  */
                            /* (the fixed-entropy router fused in)                              */

/* Flag, OR-ed into the one enumerated argument of dvq_route_select_dual_f32 / dvq_route_select_triple_f32 (`gate_dtype`) and of
 * dvq_router_gate_f32 (`activation`), the way DVQ_MODE_WS_CLEAN rides on `mode`: the BRANCH FEATURES (h_coarse, h_median, h_fine,
 * and h_out of the selects) are fp16 or bf16 -- DVQ_FEATURES(DVQ_DTYPE_F16) / DVQ_FEATURES(DVQ_DTYPE_BF16), defined with the *_x16
 * entry points below -- as an encoder under autocast produces them.  The contract is that of the *_x16 assign, carried through the
 * routing tail: every integer output (indices, the argmax behind them) is what the float32 op gives on the widened features; the
 * gate logits and cmask stay float32; h_out holds exactly the selected 16-bit values (a select moves bytes and rounds nothing).
 * The enumerator is the low byte and is checked where and with the words it always was; dtype bits other than 0 (float32), 1, 2
 * are DVQ_EINVAL.  Every other entry point refuses the flag by its own enumerator check. */
#define DVQ_FEATURES(dtype) ((dtype) << 8)

/* Flag, OR-ed into the same argument of the same three entry points, alone or together with DVQ_FEATURES(dtype): the branch features
 * are CHANNELS_LAST.  Every branch (h_coarse, h_median, h_fine) and h_out of the selects is [B, rows, cols, C] row-major -- the bytes
 * of a torch.channels_last tensor -- instead of [B, C, rows, cols]; shapes, indices, cmask (one channel: the same bytes in both
 * layouts) and the gate logits are unchanged.  The selects move a pixel's run of C elements in pieces of 16, 8, 4 or 2 bytes, as
 * the run's length and the actual alignment of the four tensors allow (DVQ_EUNSUPPORTED for 16 * wc * C >= 2^31); h_out holds
 * exactly the selected values.  The router gate reads the branches in place: its pooled averages are the bits of the NCHW form,
 * its GroupNorm sums are added in another (fixed) order, so the logits agree with the NCHW form's within rounding, not bit for bit;
 * on 16-bit features they are the float32 DVQ_NHWC op's on the widened values, bit for bit.  Branches must be aligned to their
 * element size (DVQ_EINVAL); dvq_router_gate_workspace_bytes / _prep_bytes do not depend on the layout.
 * The argument as a whole: enumerator = low byte, dtype = bits 8 - 11, layout = bit 12; a bit above 12 in a non-negative value is
 * DVQ_EINVAL.  dvq_route_select_dual_entropy_f32 has no argument that can carry a flag (run dvq_entropy_gate_f32, then the int64
 * select); every other entry point refuses the flag by its own enumerator check. */
#define DVQ_NHWC (1 << 12)   /* 0x1000: the bit above the four of DVQ_FEATURES(dtype) */

DVQ_API int dvq_version(void);
DVQ_API const char *dvq_last_error_string(void);

/*
 * Codebook preparation -- run once per codebook (weights change only in training).
 * Replaces: codebook_t.pow(2).sum(0)  (quantize2_mask.py:31,40) /
 *           torch.sum(embedding.weight**2, dim=1) (quantize_vqgan.py:281)
 * and lays the codebook out as the LDS tile images the assign kernels stream.
 *   codebook [K, D] (for VQEmbedding pass weight[:-1]); prep: >= dvq_codebook_prep_bytes(K, D)
 */
DVQ_API size_t dvq_codebook_prep_bytes(int K, int D);
DVQ_API int dvq_codebook_prepare_f32(const float *codebook, int K, int D,
                             void *prep, size_t prep_bytes, void *stream);

/*
 * Nearest-codebook assignment + quantised latents + commitment-loss sum.
 * Replaces: VectorQuantize2.forward (quantize2_mask.py:157-191: NCHW->NHWC copy,
 *           VQEmbedding.compute_distances :29-48, find_nearest_embedding :50-55,
 *           embed :130-132, masked loss :172-179, straight-through :182, NHWC->NCHW :187-189)
 *           and VectorQuantizer2.forward (quantize_vqgan.py:271-312).
 *   z        [B, D, HW]        (NCHW feature map, HW = H*W; HW == 1 is the flat [N, D] case)
 *   codebook [K, D], prep from dvq_codebook_prepare_f32 of the SAME codebook
 *   mask     nullable [B, HW]  (codebook_mask [B,1,H,W])
 *   zq       nullable [B, D, HW]   z + (e - z), two fp32 roundings like the reference
 *   codes    [B, HW] int64         first-index argmin, NaN = minimum (torch CPU semantics)
 *   loss     nullable [2] f32: loss[0] = mean((e-z)^2*mask), loss[1] = fl(fl(beta*mean)+mean)
 *   ws       >= dvq_vq_assign_workspace_bytes(...)
 * Distances follow the reference's fp32 arithmetic bit for bit: sequential-k FMA
 * chain, ATen-order norms, d = fl(fl(xn+en) - 2 dot).
 */
DVQ_API size_t dvq_vq_assign_workspace_bytes(int B, int D, int HW, int K, int mode);
DVQ_API int dvq_vq_assign_nchw_f32(const float *z, const float *codebook, const void *prep,
                           const float *mask, int B, int D, int HW, int K, float beta,
                           float *zq, int64_t *codes, float *loss,
                           void *ws, size_t ws_bytes, int mode, void *stream);

/*
 * The same op on ROW-MAJOR latents z [N, D] (a token's channels contiguous) -- what the reference builds before it calls the
 * codebook: `rearrange(x, 'b c h w -> b (h w) c')` (quantize2_mask.py:160-167; channel_last=True inputs arrive that way),
 * the concatenated item rows of VectorQuantize2List (quantize2_list.py:153-170) and VQEmbedding.forward's inputs [..., D]
 * (quantize2_mask.py:117-128).  mask nullable [N]; zq nullable [N, D]; codes [N] int64.  Equivalent to
 * dvq_vq_assign_nchw_f32 with B = N, HW = 1 (which takes the same row-major kernel form for HW == 1): in DVQ_MODE_FILTER
 * pass 1 reads and writes each row with 16-byte accesses (z and zq 16-byte aligned; otherwise, and in DVQ_MODE_EXACT,
 * lane-per-token 4-byte accesses).  Workspace: dvq_vq_assign_workspace_bytes(N, D, 1, K, mode).
 */
DVQ_API int dvq_vq_assign_flat_f32(const float *z, const float *codebook, const void *prep, const float *mask,
                           int64_t N, int D, int K, float beta, float *zq, int64_t *codes, float *loss,
                           void *ws, size_t ws_bytes, int mode, void *stream);

/* Diagnostic: byte offset inside the workspace of two int32 counters of the last DVQ_MODE_FILTER
 * call on that workspace: [0] tokens queued for the resolver (best and runner-up closer than the
 * error bound), [1] tokens handed to the full exact pass (non-finite / unscalable tokens,
 * overflow).  Read them after the stream has drained. */
DVQ_API size_t dvq_vq_assign_fallback_count_offset(int B, int D, int HW, int K);

/* nn.Embedding gather (quantize2_mask.py:130-132, get_codebook_entry :207-210):
 * out[n, :] = codebook[idx[n], :];  an index outside [0, K) writes NaNs to that row. */
DVQ_API int dvq_embed_gather_f32(const float *codebook, int K, int D, const int64_t *idx,
                         int64_t n, float *out, void *stream);

/* DualGrainFixedEntropyRouter.forward (RouterDual.py:53-57):
 * gate[i, 0] = entropy[i] <= thr, gate[i, 1] = entropy[i] > thr, int64. */
DVQ_API int dvq_entropy_gate_f32(const float *entropy, int64_t n, float thr, int64_t *gate,
                         void *stream);

/*
 * Routing tail of DualGrainEncoder.forward in eval mode (EncoderDual.py:134-149):
 * argmax over the 2 gate values, nearest x2 upsample of h_coarse, select, codebook_mask.
 *   gate [B, hc, wc, 2] (DVQ_GATE_F32 logits or DVQ_GATE_I64)
 *   h_coarse [B, C, hc, wc], h_fine [B, C, 2hc, 2wc]
 *   h_out [B, C, 2hc, 2wc], indices [B, hc, wc] int64, cmask [B, 1, 2hc, 2wc] (0.25 / 1.0)
 * h_coarse, h_fine and h_out hold float32; with gate_dtype | DVQ_FEATURES(DVQ_DTYPE_F16 / DVQ_DTYPE_BF16) they hold 2-byte elements
 * of that type (2-byte aligned, DVQ_EINVAL otherwise; h_out = the selected elements, bit for bit; any hc, wc, C).  This and the
 * triple select move the widest pieces the row length and the alignment of h_fine / h_out / cmask allow, 16 bytes at the best.
 * With gate_dtype | DVQ_NHWC (alone or with DVQ_FEATURES) h_coarse, h_fine and h_out are [B, rows, cols, C]: see DVQ_NHWC.
 */
DVQ_API int dvq_route_select_dual_f32(const void *gate, int gate_dtype,
                              const void *h_coarse, const void *h_fine,
                              int B, int C, int hc, int wc,
                              void *h_out, int64_t *indices, float *cmask, void *stream);

/* The fixed-entropy router (RouterDual.py:46-57) fused into the dual select: entropy [B, hc, wc] f32,
 * gate = [(entropy <= threshold), (entropy > threshold)]; outputs as dvq_route_select_dual_f32 plus,
 * if gate_out != NULL, the router's int64 gate [B, hc, wc, 2] (DualGrainEncoder returns it). */
DVQ_API int dvq_route_select_dual_entropy_f32(const float *entropy, float threshold, const float *h_coarse,
                                      const float *h_fine, int B, int C, int hc, int wc,
                                      float *h_out, int64_t *indices, float *cmask, int64_t *gate_out,
                                      void *stream);

/*
 * Routing tail of TripleGrainEncoder.forward in eval mode (EncoderTriple.py:148-176).
 *   gate [B, hc, wc, 3]; h_coarse [B,C,hc,wc], h_median [B,C,2hc,2wc], h_fine [B,C,4hc,4wc]
 *   cmask values 0.0625 / 0.25 / 1.0
 * h_* and h_out: float32, or 2-byte elements with gate_dtype | DVQ_FEATURES(dtype), as for dvq_route_select_dual_f32; channels_last
 * with gate_dtype | DVQ_NHWC.
 */
DVQ_API int dvq_route_select_triple_f32(const void *gate, int gate_dtype,
                                const void *h_coarse, const void *h_median,
                                const void *h_fine, int B, int C, int hc, int wc,
                                void *h_out, int64_t *indices, float *cmask, void *stream);

/*
 * Routed assignment: routing tail + VectorQuantize2.forward as ONE op straight from the encoder
 * branches -- replaces dvq_route_select_{dual,triple}_f32 followed by dvq_vq_assign_nchw_f32
 * (EncoderDual.py:134-149 / EncoderTriple.py:148-176 + quantize2_mask.py:157-191) when nothing sits
 * between select and quantizer.  The select is fused into the assign's first kernel: every OUTPUT POSITION is a
 * token, read from the branch that won its cell (the grain is derived from the gate inside the kernel), scored,
 * and written; h_dual / h_triple is never materialised and indices / cmask / gate_out come out as by-products.
 * (The 2x2 / 4x4 positions of a coarse cell are copies of one vector and so get the same code; scoring each unique
 * vector once was built and measured slower -- DESIGN.md section 8.)  Same per-token arithmetic as the dense op:
 * codes, z_q, indices, cmask identical bit for bit to select + assign, loss within 1e-5.
 *   gate      DVQ_GATE_F32 / DVQ_GATE_I64: [B, hc, wc, G]; DVQ_GATE_ENTROPY (dual only): entropy [B, hc, wc]
 *             with `threshold` (gate = [(e <= thr), (e > thr)], written to gate_out [B, hc, wc, 2] if non-NULL)
 *   h_coarse  [B, D, hc, wc]; h_median [B, D, 2hc, 2wc] (triple); h_fine [B, D, S hc, S wc], S = 2 (dual) / 4 (triple)
 *   zq        nullable [B, D, S hc, S wc]; codes [B, S hc, S wc] int64; loss nullable [2] as dvq_vq_assign_nchw_f32
 *   indices   [B, hc, wc] int64 grain index per coarse cell; cmask [B, 1, S hc, S wc] (0.0625 / 0.25 / 1.0)
 *   ws        >= dvq_vq_assign_routed_workspace_bytes(num_branches, ...), 256-byte aligned
 *   mode      DVQ_MODE_EXACT / DVQ_MODE_FILTER (/ DVQ_MODE_FILTER_PASS1)
 * hc * wc <= 1024 coarse cells per image, B <= 32768; any hc, wc (32-wide output grids, i.e. every reference
 * config, take a form that stages the coarser branches through LDS).
 */
DVQ_API size_t dvq_vq_assign_routed_workspace_bytes(int num_branches, int B, int D, int hc, int wc, int K, int mode);
DVQ_API int dvq_vq_assign_routed_dual_f32(const void *gate, int gate_kind, float threshold,
                                  const float *h_coarse, const float *h_fine,
                                  const float *codebook, const void *prep,
                                  int B, int D, int hc, int wc, int K, float beta,
                                  float *zq, int64_t *codes, float *loss,
                                  int64_t *indices, float *cmask, int64_t *gate_out,
                                  void *ws, size_t ws_bytes, int mode, void *stream);
DVQ_API int dvq_vq_assign_routed_triple_f32(const void *gate, int gate_kind,
                                    const float *h_coarse, const float *h_median, const float *h_fine,
                                    const float *codebook, const void *prep,
                                    int B, int D, int hc, int wc, int K, float beta,
                                    float *zq, int64_t *codes, float *loss,
                                    int64_t *indices, float *cmask,
                                    void *ws, size_t ws_bytes, int mode, void *stream);
/*
 * The 1x1 quant_conv of the stage-1 models (nn.Conv2d(D, D, 1): dqvae_dual_feat.py:34,66, dqvae_triple_feat.py:39,75,
 * vqgan.py:42,70) as a GEMM on the fp16 matrix cores at fp32 grade (both operands split hi + lo, three MFMAs,
 * fp32 accumulation; 2^-22 products): equal to the reference's conv within 1e-5 relative to |x||w|, not bit for bit.
 *   prepare       weight [D, D] (= conv.weight[:, :, 0, 0], row = output channel), bias nullable [D]; run once per weight
 *   dvq_qconv_f32          x [B, D, HW] -> h [B, D, HW]
 *   dvq_qconv_select_f32   the router select fused in (replaces dvq_route_select_* followed by the conv: h_dual / h_triple
 *                          is never written): gate as for the routed assign, h_coarse / h_median / h_fine the encoder
 *                          branches; outputs h [B, D, S hc, S wc] plus the select's by-products indices, cmask, gate_out
 */
DVQ_API size_t dvq_qconv_prep_bytes(int D);
DVQ_API int dvq_qconv_prepare_f32(const float *weight, const float *bias, int D, void *prep, size_t prep_bytes, void *stream);
DVQ_API int dvq_qconv_f32(const float *x, const void *prep, int B, int D, int HW, float *h, void *stream);
DVQ_API int dvq_qconv_select_f32(int num_branches, const void *gate, int gate_kind, float threshold,
                         const float *h_coarse, const float *h_median, const float *h_fine, const void *prep,
                         int B, int D, int hc, int wc, float *h, int64_t *indices, float *cmask, int64_t *gate_out,
                         void *stream);

/*
 * The model order as ONE op: [select ->] 1x1 quant_conv -> assign, with the conv as the PROLOGUE of the assign's pass 1
 * (reference: `h = self.quant_conv(h_dual)` between the routing tail and `self.quantize`, dqvae_dual_entropy.py:124-134,
 * dqvae_dual_feat.py:59-68, dqvae_triple_feat.py:68-77, vqgan.py:68-72).  Each wave computes its tokens' conv output
 * straight into the registers pass 1 keeps its latents in (same split-fp16 arithmetic as dvq_qconv_f32; the per-token
 * scale follows the running maximum of the input channels): neither h_dual / h_triple nor the conv's output is written.
 * Contract: the conv output h the op scores is within 1e-5 * sum |w||x| of the fp64 conv; codes, z_q and loss are
 * bit-exact GIVEN that h.  D = 256 and DVQ_MODE_FILTER (or DVQ_MODE_FILTER_PASS1) only -- other sizes: dvq_qconv_* followed
 * by the assign (DVQ_EUNSUPPORTED otherwise).
 *   qconv_prep   the buffer dvq_qconv_prepare_f32 filled
 *   h_buf        NULL, or with h_all != 0 [B, D, HW] floats that receive the conv output the op scored, for EVERY token (how the
 *                tests and bench.py check the contract above).  Since 0.6.0 the op needs no scratch: the tokens pass 1 or the
 *                resolver hand to the exact-list kernel (non-finite or out-of-range latents, queue or candidate overflow) get
 *                their conv output computed by that kernel, from the conv's input, with dvq_qconv_f32's arithmetic (0.3.0 -
 *                0.5.0 REQUIRED a full-size h_buf for their rows: 256 MiB per stream at B = 256).  h_all == 0: h_buf is ignored.
 *   everything else as dvq_vq_assign_nchw_f32 / dvq_vq_assign_routed_{dual,triple}_f32 (x / h_coarse.. = the conv's INPUT)
 */
DVQ_API int dvq_vq_assign_qconv_f32(const float *x, const void *qconv_prep, const float *codebook, const void *prep,
                            const float *mask, int B, int D, int HW, int K, float beta,
                            float *zq, int64_t *codes, float *loss, float *h_buf, int h_all,
                            void *ws, size_t ws_bytes, int mode, void *stream);
DVQ_API int dvq_vq_assign_routed_qconv_dual_f32(const void *gate, int gate_kind, float threshold,
                                        const float *h_coarse, const float *h_fine, const void *qconv_prep,
                                        const float *codebook, const void *prep,
                                        int B, int D, int hc, int wc, int K, float beta,
                                        float *zq, int64_t *codes, float *loss,
                                        int64_t *indices, float *cmask, int64_t *gate_out, float *h_buf, int h_all,
                                        void *ws, size_t ws_bytes, int mode, void *stream);
DVQ_API int dvq_vq_assign_routed_qconv_triple_f32(const void *gate, int gate_kind,
                                          const float *h_coarse, const float *h_median, const float *h_fine,
                                          const void *qconv_prep, const float *codebook, const void *prep,
                                          int B, int D, int hc, int wc, int K, float beta,
                                          float *zq, int64_t *codes, float *loss,
                                          int64_t *indices, float *cmask, float *h_buf, int h_all,
                                          void *ws, size_t ws_bytes, int mode, void *stream);

/*
 * The quant_conv FOLDED into the codebook -- opt-in form of the model order for callers that need no loss: loss-free
 * inference and stage 2's tokenisation, which keeps the code indices only
 * (models/stage2_dynamic/dqtransformer_uncond_entropy.py:166-171,182 around models/stage1_dynamic/dqvae_dual_entropy.py:124-134).
 * With h = W x + bias the nearest code maximises  h.e_j - en_j/2 = x.(W^T e_j) + (bias.e_j - en_j/2):  pass 1 scores the conv's
 * INPUT against the image of E W (built in float64 by dvq_fold_prepare_f32, once per codebook / conv pair) and computes NO conv;
 * only tokens it cannot prove decided get their conv output (dvq_qconv_f32's arithmetic, bit for bit) and the reference's fp32
 * distance chain on it (resolver / exact-list kernel).  The decision bound covers every h within the conv contract's tolerance
 * (1e-5 * sum |w||x| of the real-number conv), so:
 *   codes = the reference argmin (quantize2_mask.py:29-55) evaluated on h = dvq_qconv_f32(x) -- identical to
 *           dvq_qconv_f32 followed by dvq_vq_assign_nchw_f32; versus another conv implementation within that tolerance, codes can
 *           differ only at near-ties of that tolerance (as for dvq_vq_assign_qconv_f32);
 *   zq    = nullable; codebook[code] for the tokens pass 1 / the resolver decide, fl(h + fl(e - h)) for the few the exact-list
 *           kernel handles: within 1e-6 relative of the reference's z_q given h (north_star tolerance 1e-5);
 *   no loss (the conv output of a decided token is never formed; use dvq_vq_assign_*qconv* when the loss is needed).
 * dvq_fold_prepare_f32: codebook [K, D] and ITS prep (dvq_codebook_prepare_f32), conv_weight [D, D] (row = output channel),
 * conv_bias nullable [D] -> fold_prep (>= dvq_fold_prep_bytes(K, D), 256-byte aligned).  qconv_prep: dvq_qconv_prepare_f32 of the
 * same weight / bias.  D in {64, 128, 256}.  Workspaces: dvq_vq_assign_workspace_bytes(.., DVQ_MODE_FILTER) /
 * dvq_vq_assign_routed_workspace_bytes; dvq_vq_assign_*fallback_count_offset apply.  mode: DVQ_MODE_FILTER (or
 * DVQ_MODE_FILTER_PASS1, the profiling aid).  Other arguments as the qconv forms.
 */
DVQ_API size_t dvq_fold_prep_bytes(int K, int D);
DVQ_API int dvq_fold_prepare_f32(const float *codebook, int K, int D, const void *codebook_prep, const float *conv_weight,
                         const float *conv_bias, void *fold_prep, size_t fold_prep_bytes, void *stream);
DVQ_API int dvq_vq_assign_fold_f32(const float *x, const void *qconv_prep, const void *fold_prep, const float *codebook,
                           const void *prep, int B, int D, int HW, int K, float *zq, int64_t *codes,
                           void *ws, size_t ws_bytes, int mode, void *stream);
DVQ_API int dvq_vq_assign_routed_fold_dual_f32(const void *gate, int gate_kind, float threshold,
                                       const float *h_coarse, const float *h_fine, const void *qconv_prep,
                                       const void *fold_prep, const float *codebook, const void *prep,
                                       int B, int D, int hc, int wc, int K, float *zq, int64_t *codes,
                                       int64_t *indices, float *cmask, int64_t *gate_out,
                                       void *ws, size_t ws_bytes, int mode, void *stream);
DVQ_API int dvq_vq_assign_routed_fold_triple_f32(const void *gate, int gate_kind,
                                         const float *h_coarse, const float *h_median, const float *h_fine,
                                         const void *qconv_prep, const void *fold_prep, const float *codebook, const void *prep,
                                         int B, int D, int hc, int wc, int K, float *zq, int64_t *codes,
                                         int64_t *indices, float *cmask, void *ws, size_t ws_bytes, int mode, void *stream);
/* audit aid, as dvq_debug_filter_scores_f32 for the folded image: tokens = the conv's inputs [n, D]; scores G'_j, the per-token
 * threshold 2W' (which also covers the conv tolerance), ||x||^2 and the scale 2^b' */
DVQ_API int dvq_debug_fold_scores_f32(const float *tokens, int n, const void *fold_prep, int D, int K, float *scores,
                              float *threshold, float *xn, float *scale, void *stream);

/*
 * Backward of the quantizer's forward with respect to its input -- what autograd derives from the reference graph
 * (quantize2_mask.py:172-182, quantize_vqgan.py:290-298): identity through z + (z_q - z).detach() plus the commitment term,
 *   g_z = g_zq + (g_loss * coef_scale) * ((z - e) * mask),   e = codebook[codes]  (the codebook AS IT WAS at forward time:
 *   callers keep a snapshot, the EMA update rewrites the weight between forward and backward), coef_scale = 2 c / numel.
 * One streaming pass (the reference: five or six element-wise passes and a transposed copy of e); same fp32 operation order
 * as that expression.  g_zq nullable (only the loss was used), g_loss nullable (only z_q was used; a device scalar otherwise),
 * mask nullable; D % 16 == 0 (DVQ_EUNSUPPORTED otherwise); codebook 16-byte aligned (DVQ_EINVAL).
 * HW == 1 is the ROW-MAJOR form, z / g_zq / g_z [N, D] with B = N (token rows, or a channels_last image map [B, C, H, W] with
 * N = B H W): since 0.18.0 a lane then owns 16-byte pieces of a token's row instead of one token at a channel stride of HW, provided z,
 * g_zq and g_z are 16-byte aligned (what torch allocates; a view at another offset is served by the strided kernel, an order of
 * magnitude slower at HW == 1).  The same bits either way.
 */
DVQ_API int dvq_vq_backward_nchw_f32(const float *z, const float *codebook, const int64_t *codes, const float *mask,
                             const float *g_zq, const float *g_loss, float coef_scale,
                             int B, int D, int HW, int K, float *g_z, void *stream);
/* ... and with respect to a codebook trained by back-propagation (VectorQuantizer2, quantize_vqgan.py:290-298; no EMA):
 *   g_weight[j, :] += -(g_loss * coef_scale) * sum over tokens with code j of (z - codebook[j]) * mask
 * ACCUMULATES into g_weight [>= K rows, D] (zero it first); float atomics, one row per distinct code of a 64-token tile:
 * equal to the reference's index_add_ of the [N, D] differences up to summation order.  K <= 8192 (DVQ_EUNSUPPORTED above).
 * HW == 1 (row-major z [N, D], B = N; since 0.18.0): a wave reads 64 consecutive channels of a token straight from its row, any D, any
 * 4-byte aligned z; the K limit stays part of the contract although that kernel needs no table. */
DVQ_API int dvq_vq_backward_codebook_nchw_f32(const float *z, const float *codebook, const int64_t *codes, const float *mask,
                                      const float *g_loss, float coef_scale, int B, int D, int HW, int K,
                                      float *g_weight, void *stream);

/* Audit aid (tools/bound_audit.py, tests/test_bound_audit.py): the pass-1 score arithmetic of DVQ_MODE_FILTER on
 * n tokens given as rows [n, D] -- every fp16-MFMA score G_j ~ -2^(b-1) (d_j - xn) as pass 1 sees it (index bits
 * packed into the low mantissa bits), the per-token decision threshold 2W, the exact norm xn and the codebook scale
 * 2^b -- so that the bound |G_j - truth_j| <= W can be checked against the reference arithmetic in float64 on the host.
 *   scores [n, 32*ceil(K/32)] (padding codes hold -3e38), threshold [n], xn [n], scale [1] (nullable) */
DVQ_API int dvq_debug_filter_scores_f32(const float *tokens, int n, const void *prep, int D, int K, float *scores,
                                float *threshold, float *xn, float *scale, void *stream);

/* as dvq_vq_assign_fallback_count_offset, for a routed workspace */
DVQ_API size_t dvq_vq_assign_routed_fallback_count_offset(int num_branches, int B, int D, int hc, int wc, int K);

/*
 * Training-mode codebook statistics, the dense part of VQEmbedding._update_buffers
 * (quantize2_mask.py:66-84: one-hot [K, N] matrix, row sum, matmul):
 *   cluster_size[j] = #tokens with code j, vectors_sum[j, :] = sum of those tokens' vectors.
 * z [B, D, HW] f32 (NCHW), codes [B, HW] int64; both outputs are overwritten.  Codes outside
 * [0, K) are ignored.  Float atomics: equal to the reference within rounding (1e-5).
 * Equal codes of a 64-token tile are summed before the atomics up to K = 8192; float32 latents with B * HW >= 65536, K <= 4096,
 * D % 16 == 0 and HW % 4 == 0 take a 2048-token tile sorted by code.  HW == 1 (row-major z [N, D], B = N; since 0.18.0): rows are read
 * where they lie (any D, z aligned to its element), equal codes are summed at every K, and the sorted tile applies to float32 rows
 * with N >= 65536, K <= 4096, D % 16 == 0 and a 16-byte aligned z.  dvq_ema_accumulate_nchw_x16 follows the same rules, without the sorted tile.
 */
DVQ_API int dvq_ema_accumulate_nchw_f32(const float *z, const int64_t *codes, int B, int D, int HW, int K,
                                float *cluster_size, float *vectors_sum, void *stream);

/*
 * Dead-code restart of the training-mode codebook update: the reference takes the first K entries of torch.randperm(n_vectors)
 * as the input vectors that replace dead codes (quantize2_mask.py:93-96) -- on a GPU a full sort of n keys to keep K of them.
 * out [k] int64 = k DISTINCT indices of [0, n), every index equally likely, in random order (the distribution of a permutation's
 * prefix: independent draws, first occurrences kept), a pure function of (seed, n, k); one small workgroup.
 * 1 <= k <= 2048, 16 k <= n < 2^32.  RNG parity with torch is not possible either way.
 * (Distinctness is a practical, not a formal property: the kernel makes 2 k draws; should fewer than k different values occur among
 * them -- probability below 1e-100 for n >= 16 k -- a slot that stayed empty keeps its own index i, which may repeat a chosen one.)
 */
DVQ_API int dvq_restart_pick_i64(uint64_t seed, int64_t n, int k, int64_t *out, void *stream);

/*
 * The rest of the training-mode codebook update as ONE kernel (quantize2_mask.py:89-115; ~20 small torch kernels in the reference):
 *   cluster_size' = cluster_size_ema * decay + (1 - decay) * stats_count          (:89)
 *   embed_ema     = embed_ema * decay + (1 - decay) * stats_sum                   (:90)
 *   restart != 0: codes with cluster_size' < 1 take their restart row and count 1   (:102-105)
 *   n = sum(cluster_size'); weight[j, :] = embed_ema[j, :] / (n * (cluster_size'[j] + eps) / (n + K * eps))   (:107-115)
 * stats_sum [K, D] / stats_count [K]: this step's statistics (dvq_ema_accumulate_nchw_f32, all-reduced by the caller).
 * cluster_size_ema [K] is READ, the new counts go to cluster_size_out [K] (must not alias: every workgroup sums the old counts;
 * copy it over the buffer afterwards); embed_ema [K, D] is updated in place; weight: rows 0 .. K-1 of a [>= K, D] tensor are written.
 * restart: 0 none; 1 rows from restart_rows [K, D] (data-parallel: rank 0's, broadcast by the caller); 2 rows gathered from the NCHW
 * latents z [B, D, HW] at token index pick[j] in [0, B * HW) (dvq_restart_pick_i64).  fp32, the reference's operation order; the sum n is
 * accumulated in double: equal to the reference within rounding (1e-5).  The reference's `1 - decay` is a Python double rounded to
 * fp32 afterwards: it is formed from the shortest decimal that rounds to the fp32 `decay` received (0.99f -> 1 - 0.99 -> 0.01f).
 */
DVQ_API int dvq_ema_update_f32(const float *stats_sum, const float *stats_count, float decay, float eps, int K, int D,
                               const float *cluster_size_ema, float *cluster_size_out, float *embed_ema, float *weight,
                               int restart, const float *restart_rows, const float *z, int B, int HW, const int64_t *pick, void *stream);

/*
 * Code-usage statistics of a batch of codes, one sweep (code_stats.hip).  Replaces what VectorQuantizer / EMAVectorQuantizer build
 * through a dense one-hot matrix (quantize_vqgan.py:58-60, 84-85 / :434-436: zeros + scatter_ or F.one_hot, mean(0), log, sum, exp) and
 * the host-side sets of scripts/tools/codebook_usage*.py.
 *   codes [N] int64 (may be NULL when N == 0); codes outside [0, K) are ignored (counted nowhere; their one-hot row is all zero).
 *   counts [K] int64      exact: counts[j] = #n with codes[n] == j
 *   n_used [1] int64      #j with counts[j] > 0
 *   perplexity [1] f32    p_j = (float)counts[j] / (float)N (one fp32 division), t_j = p_j * logf(p_j + 1e-10f), H = sum of the t_j in
 *                         double in one fixed order, perplexity = expf((float)(-H)): a pure function of the counts, the same bits on
 *                         every run; within 1e-5 relative of the reference's exp(-sum(e_mean * log(e_mean + 1e-10))).  N == 0: 1.
 *   onehot [N, K] f32     nullable; onehot[n, j] = codes[n] == j ? 1 : 0, every element written exactly once (16-byte non-temporal
 *                         stores when K % 4 == 0 and the pointer is 16-byte aligned, 4-byte stores otherwise).
 * All outputs are overwritten (the zeroing is part of the call); at most three kernel launches, no memset node, no host
 * synchronisation, capturable in a HIP graph.  Integer atomics only: the counts do not depend on arrival order.
 * DVQ_EINVAL: null counts / n_used / perplexity, null codes with N > 0, K < 1, N < 0.  DVQ_EUNSUPPORTED: K >= 2^20.
 */
DVQ_API int dvq_code_stats_f32(const int64_t *codes, int64_t N, int K, int64_t *counts, int64_t *n_used, float *perplexity,
                               float *onehot, void *stream);

/*
 * The same statistics per GRAIN of a dual (G = 2) or triple (G = 3) granularity model: codes [B, H, W] int64, grain [B, hc, wc] int64 with
 * values in [0, G), 0 = the coarsest (what the encoders return as `indices`).  H / hc == W / wc == 2^(G - 1) exactly (DVQ_EINVAL otherwise).
 * Every region of the token stream is counted once, as the permuter emits it: with s = (H / hc) >> g for the cell's grain g, position
 * (y, x) is counted iff y % s == 0 and x % s == 0, into row g.  Cells whose grain is outside [0, G) are ignored.
 *   counts [G, K] int64, n_tokens [G] int64 (regions of that grain, whatever their code), n_used [G] int64, perplexity [G] f32 with
 *   p = count / n_tokens[g]; a grain without tokens has n_used 0 and perplexity 1 (no 0 / 0).
 * Launch properties and code range as dvq_code_stats_f32.  DVQ_EINVAL: null pointer, B / hc / wc / K < 1, G not 2 or 3, the shape rule.
 * DVQ_EUNSUPPORTED: K >= 2^20 or B * H * W >= 2^31.
 */
DVQ_API int dvq_code_stats_grain_f32(const int64_t *codes, const int64_t *grain, int B, int H, int W, int hc, int wc, int G, int K,
                                     int64_t *counts, int64_t *n_tokens, int64_t *n_used, float *perplexity, void *stream);

/*
 * Fused feature-router gate (inference), the forward of DualGrainFeatureRouter
 * (modules/dynamic_modules/RouterDual.py:35-43) and TripleGrainFeatureRouter
 * (modules/dynamic_modules/RouterTriple.py:46-56): GroupNorm per branch, average pooling of the
 * finer branches onto the coarse grid, channel concat (coarse, [median,] fine), then
 *   activation == DVQ_ACT_NONE : gate = w2 x + b2                (gate_type "1layer-fc"; w1/b1 ignored,
 *                                                                 w2 is [nb, nb*C], hidden ignored)
 *   DVQ_ACT_SILU / DVQ_ACT_RELU: gate = w2 act(w1 x + b1) + b2   ("2layer-fc-SiLu" / "2layer-fc-ReLu";
 *                                                                 w1 [hidden, nb*C], w2 [nb, hidden])
 * num_branches nb = 2 (h_median must be NULL; h_fine is 2x the coarse grid) or 3 (median 2x, fine 4x).
 * h_* are [B, C, rows, cols] f32 NCHW; num_groups == 0 means normalization_type "none" (gn_* ignored),
 * otherwise gn_w_* / gn_b_* are the [C] affine parameters of each branch's GroupNorm(num_groups, C, eps).
 * gate [B, hc, wc, nb] f32 logits.  C % 8 == 0, nb*C <= 1280 and, with Fp = nb*C rounded up to 16 and
 * H = hidden (32 for DVQ_ACT_NONE), 128 * Fp + 4 * (1 + nb) * H <= 163584: the feature tile of 32 cells and
 * the output-layer rows share one workgroup's LDS.  (Exempt: a hidden layer behind GroupNorms whose groups
 * are 8, 16, ... 64 channels with nb * (C / num_groups) * hc * wc * 4 <= 49152 and nb*C one of 128, 256, 384,
 * 512 (nb = 2) or 192, 384, 768 (nb = 3) -- that form keeps the weights in registers, any hidden width.)
 * DVQ_EUNSUPPORTED names the bytes needed otherwise, and dvq_router_gate_workspace_bytes returns 0.
 * The hidden layer runs on the fp16 matrix
 * cores with both operands split hi + lo (hi*hi + hi*lo + lo*hi, fp32 accumulation: 2^-22 products);
 * summation order differs from ATen/MKL: logits equal the reference within 1e-4, not bit for bit.
 */
#define DVQ_ACT_NONE 0
#define DVQ_ACT_SILU 1
#define DVQ_ACT_RELU 2
/* The workspace holds the GroupNorm statistics and the per-cell averages of every branch (B * nb*C * hc*wc floats): the
 * features are read from HBM once.  w1_prep (nullable): the split fp16 tile images of w1 made by
 * dvq_router_gate_prepare_f32 into a caller-kept buffer of dvq_router_gate_prep_bytes -- valid while w1 is unchanged;
 * NULL: they are rebuilt inside the call. */
DVQ_API size_t dvq_router_gate_workspace_bytes(int num_branches, int B, int C, int hc, int wc, int num_groups, int hidden);
DVQ_API size_t dvq_router_gate_prep_bytes(int num_branches, int C, int hidden);
DVQ_API int dvq_router_gate_prepare_f32(const float *w1, int num_branches, int C, int hidden, void *w1_prep,
                                size_t w1_prep_bytes, void *stream);
/* Optional, after dvq_router_gate_prepare_f32 into the same buffer and again whenever a GroupNorm parameter changes: the
 * per-branch maxima of |weight| and |bias| of the branches' GroupNorms go into the buffer's tail; the gate's pooling pass then
 * derives the fp16 range of its operand images from six scalars instead of scanning all num_branches * C parameters in every
 * workgroup (-5 us of 83 at B = 128, -39 of 534 at B = 1024, triple).  Same results (the scale is an exact power of two). */
DVQ_API int dvq_router_gate_prepare_norm_f32(int num_branches, int C, int hidden,
                                     const float *gn_w_coarse, const float *gn_b_coarse,
                                     const float *gn_w_median, const float *gn_b_median,
                                     const float *gn_w_fine, const float *gn_b_fine,
                                     void *w1_prep, size_t w1_prep_bytes, void *stream);
/* h_*: float32; with activation | DVQ_FEATURES(DVQ_DTYPE_F16 / DVQ_DTYPE_BF16) 2-byte elements of that type (8-byte aligned, DVQ_EINVAL
 * otherwise), widened to float32 where the pooling pass loads them: the logits are those of this op on the widened features, bit for
 * bit.  Workspace, prep and every other argument are the same (dvq_router_gate_workspace_bytes takes no dtype).
 * With activation | DVQ_NHWC (alone or with DVQ_FEATURES) the branches are [B, rows, cols, C], aligned to their element size: see
 * DVQ_NHWC. */
DVQ_API int dvq_router_gate_f32(int num_branches, const void *h_coarse, const void *h_median, const void *h_fine,
                        int B, int C, int hc, int wc, int num_groups, float eps,
                        const float *gn_w_coarse, const float *gn_b_coarse,
                        const float *gn_w_median, const float *gn_b_median,
                        const float *gn_w_fine, const float *gn_b_fine,
                        const float *w1, const float *b1, const float *w2, const float *b2,
                        int hidden, int activation, const void *w1_prep, float *gate, void *ws, size_t ws_bytes,
                        void *stream);

/*
 * Training-mode routing tail of the feature routers and its backward (DualGrainEncoder.forward with update_router,
 * EncoderDual.py:131-156; TripleGrainEncoder.forward in training, EncoderTriple.py:145-183), differentiable into the branches
 * and every router parameter.  Router arguments as dvq_router_gate_f32 (hidden = 0 and w1 = b1 = NULL with DVQ_ACT_NONE:
 * w2 [nb, nb*C] is the single Linear); same shape limits.  Forward:
 *   logits = gate MLP(concat(pool(GroupNorm(h_*))));  with gumbels ([B, hc, wc, nb] f32, the noise F.gumbel_softmax draws):
 *   y = softmax((logits + gumbels) / tau), k = first max of y, gate_j = (onehot_j - y_j) + y_j (the reference's rounding:
 *   0 off k), indices = argmax gate, h_out = select(indices) * gate_k, codebook_mask as dvq_route_select_*_f32.
 *   gumbels == NULL (no-gumbel mode, the dual encoder with update_router=False): gate = logits, h_out = select(indices).
 * h_out is [B, C, S hc, S wc] (S = 2 dual, 4 triple), indices [B, hc, wc], codebook_mask [B, 1, S hc, S wc], gate [B, hc, wc, nb].
 * The workspace (dvq_route_train_workspace_bytes, 256-byte aligned) holds the saved activations: the caller keeps it unchanged
 * from the forward to the backward of the same arguments (the backward also uses it as scratch beyond the saved part).
 * Backward: g_out = d h_out, g_gate = d gate (either nullable = zero) -> dh_* (the branches' full gradients), the GroupNorm
 * affine gradients dgn_* (NULL / ignored when num_groups == 0), dw1 / db1 (2-layer gates), dw2 / db2; every output overwritten.
 * All arithmetic fp32 (matrix products on the fp32 matrix cores); every reduction over cells runs in a fixed order: the outputs are
 * bitwise reproducible run to run.  tau > 0; S * wc <= 4096; B * C * (S hc) * (S wc) < 2^31.
 */
DVQ_API size_t dvq_route_train_workspace_bytes(int num_branches, int B, int C, int hc, int wc, int num_groups, int hidden);
DVQ_API int dvq_route_train_forward_f32(int num_branches, const float *h_coarse, const float *h_median, const float *h_fine,
                                int B, int C, int hc, int wc, int num_groups, float eps,
                                const float *gn_w_coarse, const float *gn_b_coarse,
                                const float *gn_w_median, const float *gn_b_median,
                                const float *gn_w_fine, const float *gn_b_fine,
                                const float *w1, const float *b1, const float *w2, const float *b2,
                                int hidden, int activation, const float *gumbels, float tau,
                                float *h_out, int64_t *indices, float *codebook_mask, float *gate,
                                void *ws, size_t ws_bytes, void *stream);
DVQ_API int dvq_route_train_backward_f32(int num_branches, const float *h_coarse, const float *h_median, const float *h_fine,
                                 int B, int C, int hc, int wc, int num_groups, float eps,
                                 const float *gn_w_coarse, const float *gn_b_coarse,
                                 const float *gn_w_median, const float *gn_b_median,
                                 const float *gn_w_fine, const float *gn_b_fine,
                                 const float *w1, const float *b1, const float *w2, const float *b2,
                                 int hidden, int activation, const float *gumbels, float tau,
                                 const float *g_out, const float *g_gate, void *ws, size_t ws_bytes,
                                 float *dh_coarse, float *dh_median, float *dh_fine,
                                 float *dgn_w_coarse, float *dgn_b_coarse, float *dgn_w_median, float *dgn_b_median,
                                 float *dgn_w_fine, float *dgn_b_fine,
                                 float *dw1, float *db1, float *dw2, float *db2, void *stream);

/*
 * Residual quantization: RQBottleneck (modules/vector_quantization/quantize_rqvae.py:149-400) around dvq_vq_assign_flat_f32.
 * Geometry: x is the latent [B, H, W, Dl] channel-last (RQVAE.encode, models/stage1/rqvae.py:112-115), the code grid is
 * h x w with H = h rH, W = w rW, N = B h w tokens of D = rH rW Dl channels (to_code_shape :216-224: code element (n, j) of
 * token n = (b, hh, ww), channel j = (a rW + c) Dl + l, is latent element (b, hh rH + a, ww rW + c, l)).  D a multiple of 32,
 * at most 256 (the widths the assign serves, with zero padding below 256; DVQ_EUNSUPPORTED otherwise); Dl rH rW == D;
 * N D < 2^31; 1 <= depth <= DVQ_RQ_MAX_DEPTH.  quantize :237-271 as one caller loop, i = 0 .. depth-1:
 *   dvq_vq_assign_flat_f32(r_i, E_i, ..., zq = NULL, codes = c_i [N], loss = NULL)   (r_0 = x in code layout)
 *   dvq_rq_step_f32(.., r_i, E_i, c_i, i, ..)
 *   (training) the EMA update of codebook i on (r_i, c_i) -- it reads r_i, so r_{i+1} lives in the other residual slot
 * then dvq_rq_loss_f32.  The workspace (dvq_rq_workspace_bytes(N, D, depth, want_grad), 256-byte aligned) holds the loss
 * partials, two residual slots, agg and (want_grad) s; r_i for i >= 1 is at byte dvq_rq_residual_offset(N, D, depth, i) of it
 * (0 = no such residual).  With rH = rW = 1, r_0 is x itself; otherwise the caller passes one code-layout copy of x.
 * Step i, per element, in this fp32 order (e = E_i[c_i], agg_0 = +0):
 *   agg_{i+1} = fl(agg_i + e);  r_{i+1} = fl(r_i - e) (not on the last depth);  d = fl(x - agg_{i+1});
 *   loss partial += fl(d d) in double, summed per block in a fixed order;  want_grad: s = d (i = 0), fl(s + d) (i > 0);
 *   codes[n, i] = c_i  (codes [N, depth] int64);  last depth: out = fl(x + fl(agg_d - x)) in latent layout (forward :273-281),
 *   instead of agg.  A code outside [0, K) gathers NaN.
 * dvq_rq_loss_f32: loss[0] = fl(sum_i fl32(S_i / (N D)) / depth), S_i the partials of depth i in block order
 *   (compute_commitment_loss :283-296, mean(stack(means))).  Bitwise reproducible run to run.
 * dvq_rq_backward_f32: g_x = fl(g_out + fl(fl(g_loss[0] fl32(2 / (N D depth))) s)) in latent layout (g_out / g_loss nullable =
 *   zero): the straight-through identity plus d loss / d x; the codebooks are EMA buffers and get no gradient.  Needs the
 *   want_grad workspace of the forward, unchanged since.
 * dvq_rq_embed_code_f32: codebooks / K = HOST arrays of `depth` device pointers / row counts (the reference's embed reads the
 *   padding row too: pass K = n_embed + 1); codes [B h w, depth] int64; j < depth; out in latent layout:
 *   DVQ_RQ_EMBED_SUM     out = fl(...fl(fl(0 + e_0) + e_1)... + e_j)   [B, H, W, Dl]  (embed_code :298-311 for j = depth-1,
 *                        embed_partial_code 'add' :337-369)
 *   DVQ_RQ_EMBED_SELECT  out = e_j                                   [B, H, W, Dl]  (embed_partial_code 'select')
 *   DVQ_RQ_EMBED_EACH    out[.., t, :] = e_t, t <= j               [B, H, W, j+1, Dl]  (embed_code_with_depth :314-334;
 *                        rH = rW = 1, Dl = D gives its code-layout form)
 *   a code outside [0, K_t) writes a NaN row.
 */
#define DVQ_RQ_MAX_DEPTH     16
#define DVQ_RQ_EMBED_SUM      0
#define DVQ_RQ_EMBED_SELECT   1
#define DVQ_RQ_EMBED_EACH     2
DVQ_API size_t dvq_rq_workspace_bytes(int64_t N, int D, int depth, int want_grad);
DVQ_API size_t dvq_rq_residual_offset(int64_t N, int D, int depth, int i);
DVQ_API int dvq_rq_step_f32(const float *x, const float *r, const float *codebook, int K, const int64_t *code,
                            int B, int h, int w, int rH, int rW, int Dl, int D, int i, int depth, int want_grad,
                            int64_t *codes, float *out, void *ws, size_t ws_bytes, void *stream);
DVQ_API int dvq_rq_loss_f32(int64_t N, int D, int depth, const void *ws, size_t ws_bytes, float *loss, void *stream);
DVQ_API int dvq_rq_backward_f32(const float *g_out, const float *g_loss, int B, int h, int w, int rH, int rW, int Dl, int D,
                                int depth, const void *ws, size_t ws_bytes, float *g_x, void *stream);
DVQ_API int dvq_rq_embed_code_f32(const float *const *codebooks, const int *K, int depth, const int64_t *codes,
                                  int B, int h, int w, int rH, int rW, int Dl, int D, int mode, int j, float *out,
                                  void *stream);

/*
 * Patch-entropy map, Entropy.forward (models/stage1_dynamic/dqvae_dual_entropy.py:13-63) with
 * patch_size 16: images [B, 3, H, W] f32 (H, W multiples of 16) -> out [B, H/16, W/16] f32.
 * Transcendental fp32 math: equal to the reference within 1e-5, not bit for bit.
 */
DVQ_API int dvq_entropy_map_f32(const float *images, int B, int H, int W, int patch, float *out, void *stream);

/*
 * DualGrainSeperatePermuter (modules/dynamic_modules/permuter.py): dense codes + grain map <->
 * variable-length coarse / fine streams.  All tensors int64 like the reference.
 *   count    counts[B,2] = (#coarse, #fine cells) per image, maxes[2] = their batch maxima; the
 *            caller reads maxes (one device->host copy, as pad_sequence implies) and allocates
 *            Lc = maxes[0] + 1, Lf = 4*maxes[1] + 1.
 *   forward  permuter.py:50-109.  codes [B, 2hc, 2wc], grain [B, hc, wc] (0 coarse / 1 fine),
 *            order 0 = "region-first", 1 = "row-first"; special[6] (HOST array) = content_pad,
 *            content_eos, coarse_position_pad, coarse_position_eos, fine_position_pad,
 *            fine_position_eos; outputs [B, Lc] x3 (content, position, segment = 0) and [B, Lf] x3
 *            (content, position, segment = 1).  Entries that do not fit Lc / Lf are dropped.
 *   backward permuter.py:111-135 (sequential semantics: later entries win, entries after EOS
 *            ignored, no coarse upsample if the coarse stream has no EOS) -> target [B, 2hc, 2wc].
 * hc*wc <= 1024.
 */
DVQ_API int dvq_permute_dual_count_i64(const int64_t *grain, int B, int hc, int wc,
                               int32_t *counts, int32_t *maxes, void *stream);
DVQ_API int dvq_permute_dual_forward_i64(const int64_t *codes, const int64_t *grain, int B, int hc, int wc,
                                 int order, int Lc, int Lf, const int64_t *special,
                                 int64_t *coarse_content, int64_t *coarse_position, int64_t *coarse_segment,
                                 int64_t *fine_content, int64_t *fine_position, int64_t *fine_segment,
                                 void *stream);
DVQ_API int dvq_permute_dual_backward_i64(const int64_t *coarse_content, const int64_t *fine_content,
                                  const int64_t *coarse_position, const int64_t *fine_position,
                                  int B, int Lc, int Lf, int hc, int wc,
                                  int64_t coarse_position_eos, int64_t fine_position_eos,
                                  int64_t *target, void *stream);

/*
 * Stage-2 sampling (Dualformer.sample_from_scratch, models/stage2_dynamic/dqtransformer_{class,class2_entropy,uncond_entropy}.py).
 *
 * dvq_sample_head_f32: ONE sampling step for all B rows -- replaces `logits[:, -1, :] / temperature`, the avoid_* helper of
 * the step (dqtransformer_class.py:518-557), top_k_logits, F.softmax, top_p_logits (models/stage2/utils.py:22-40) and
 * torch.multinomial / torch.topk (dqtransformer_class.py:313-330 and the three other position / content blocks).  Per row b:
 *   1. x[j] = logits[b * logits_row_stride + j] / temperature (IEEE division), j < V <= 8192 (larger V: DVQ_EUNSUPPORTED).
 *      Pass the last time step of a [B, T, V] tensor as logits = base + (T-1) * V, logits_row_stride = T * V.
 *   2. the mask rule.  rules (HOST array of 7) = {pad, ban_a, ban_from, restore, ban_b, ban_from_post, flag_code}; -1 marks an
 *      unused code; pad, ban_a, restore, ban_b, flag_code must lie in [0, V) when used, ban_from / ban_from_post in [0, V]
 *      (DVQ_EINVAL otherwise).  If flag[b] != 0: out = -inf everywhere except out[pad] = x[pad].  Otherwise, in this order:
 *        out = x; out[history[b, :history_len]] = -inf (codes outside [0, V) are skipped); out[pad] = out[ban_a] = -inf;
 *        out[ban_from:] = -inf; out[restore] = x[restore]; out[ban_b] = -inf; out[ban_from_post:] = -inf.
 *      The three reference variants (max_idx = coarse_hw^2 - 1, kept as the reference has it: position max_idx is banned):
 *        coarse position (all)    {cpad, -1, max_idx, ceos, -1, -1, ceos}     history = the sampled coarse positions, sos included
 *        fine position (class,    {fpad, -1, -1, feos, fsos, -1, feos}        history = the transferred fine positions + the
 *                       uncond)                                                         sampled ones (eos and pad included)
 *        fine position (class2)   {fpad, -1, -1, feos, -1, feos + 1, feos}
 *        content (class, class2)  {pad, -1, eos, -1, -1, -1, -1}
 *        content (uncond)         {pad, eos, -1, -1, sos, -1, -1}
 *   3. top_k (0 = off, else 1..V): out[out < k-th largest] = -inf (exact radix select; ties at the threshold are all kept).
 *   4. p = softmax(out): max, expf, ONE fixed-order sum -- deterministic, within 1e-6 of torch (reduction order differs).
 *   5. top_p (0 = off, else (0, 1]): order the row by p descending, equal p by ASCENDING index; keep an element iff the mass
 *      of the elements strictly before it is < top_p (the first is always kept; masses in 48-bit fixed point), zero the
 *      rest, p = p / sum(kept).
 *   6. the token: sample != 0: argmax_j p[j] / q[b * V + j], q = caller-drawn Exp(1) variates [B, V] (what torch.multinomial
 *      computes from its own exponential_ draw); sample == 0: argmax_j p[j]; the first index on ties.
 *   7. tokens[b * tokens_row_stride] = token (int64; point tokens at column t of a [B, L] sequence buffer to append);
 *      flag[b] += (token == flag_code) when flag_code >= 0 (flag: float32 [B], the reference's [B, 1] flag tensor);
 *      out_logits / out_probs (nullable, [B, V]) receive out after step 3 and p after step 5.
 *   No host synchronisation, no allocation: capturable in a HIP graph.
 *
 * Position transfer, transfer_sampled_coarse_position_to_{sampled,remain}_fine_position (dqtransformer_class.py:464-516):
 *   coarse_position [B, Lc] (row stride >= Lc): column 0 the sos, then sampled coarse cells up to the first coarse EOS (cells
 *   outside [0, hc*hc) are skipped, repeats mark one cell).  variant DVQ_TRANSFER_SAMPLED marks those cells,
 *   DVQ_TRANSFER_REMAIN the others.
 *   count  counts[b] = marked cells of row b, *max_count = their batch maximum (one int the caller may read back:
 *          L = (sos_mode != NONE) + 4 * max_count + 1 is the width pad_sequence gives).
 *   fill   out [B, L]: [sos] + the fine positions of the marked cells in `order` (0 region-first: the 4 positions of each
 *          cell together, cells row-major; 1 row-first: fine pixels row-major), as position_sequence_fine[...] lists them,
 *          then fine_position_eos, then fine_position_pad.  sos_mode DVQ_TRANSFER_SOS_CONST writes sos_code (class, uncond),
 *          DVQ_TRANSFER_SOS_COPY copies coarse_position[b, 0] (class2_entropy :468, :496), DVQ_TRANSFER_SOS_NONE none
 *          (activate_sos_for_fine_sequence = False).  Entries beyond L are dropped.
 *   hc * hc <= 1024 coarse cells of 2 x 2 fine positions each (fine_hw = 2 * coarse_hw, as the permuter; the Python
 *   SamplingRules rejects other ratios).  Integer work: bit-exact.
 */
#define DVQ_TRANSFER_SAMPLED   0
#define DVQ_TRANSFER_REMAIN    1
#define DVQ_TRANSFER_SOS_NONE  0
#define DVQ_TRANSFER_SOS_CONST 1
#define DVQ_TRANSFER_SOS_COPY  2
DVQ_API int dvq_sample_head_f32(const float *logits, int64_t logits_row_stride, int B, int V, float temperature,
                                const int64_t *rules, const int64_t *history, int64_t history_row_stride, int history_len,
                                float *flag, int top_k, float top_p, int sample, const float *q, int64_t *tokens,
                                int64_t tokens_row_stride, float *out_logits, float *out_probs, void *stream);
DVQ_API int dvq_sample_transfer_count_i64(const int64_t *coarse_position, int64_t row_stride, int B, int Lc, int hc,
                                          int64_t coarse_position_eos, int variant, int32_t *counts, int32_t *max_count,
                                          void *stream);
DVQ_API int dvq_sample_transfer_fill_i64(const int64_t *coarse_position, int64_t row_stride, int B, int Lc, int hc,
                                         int64_t coarse_position_eos, int variant, int order, int sos_mode, int64_t sos_code,
                                         int64_t fine_position_eos, int64_t fine_position_pad, int L, int64_t *out,
                                         void *stream);

/*
 * Decode head: code indices -> the tensor the decoder's conv_in reads.  Replaces, after permuter.forward_back
 * (models/stage2_dynamic/dqtransformer_uncond_entropy.py:174-178; stage-1 decode_code, models/stage1_dynamic/dqvae_triple_feat.py:84-87):
 * quantize.get_codebook_entry (quantize2_mask.py:207-210), `.permute(0, 3, 1, 2)`, post_quant_conv
 * (models/stage1_dynamic/dqvae_dual_entropy.py:136-137) and the position block of Decoder.forward
 * (modules/dynamic_modules/DecoderPositional.py:109-118).
 *
 * dvq_decode_table_prepare_f32: table[r, o] = sum_k conv_weight[o, k] * codebook[r, k] + conv_bias[o], r < rows -- the 1x1 conv
 * applied to every codebook row once (it acts per pixel, so conv(E[code]) is row `code` of this table).  `rows` is the row count of
 * the weight tensor handed in: K + 1 for VQEmbedding (its padding row is a valid index of get_codebook_entry), K for
 * VectorQuantizer2.  fp32: one fmaf chain per output, k ascending from 0, then one add of the bias; no atomics, the same bits every
 * run; within 1e-5 * (sum_k |w||e| + |b|) of the float64 conv.  D, C <= 1024.  table: >= dvq_decode_table_bytes(rows, C), 16-byte
 * aligned.  conv_weight == NULL (then conv_bias == NULL and C == D): there is no conv, nothing is built or written -- hand the
 * codebook itself to dvq_decode_head_f32 as its table.  Run once per (codebook, conv) pair.
 *
 * dvq_decode_head_f32: h_in[b, c, p] = fl(fl(table[codes[b, p], c] + pos_first[c, p]) + pos_second[c, p]), p < HW -- the two adds
 * round as the reference's two position modules do; an add whose table is NULL is skipped.
 *   codes [B, HW] int64; a code outside [0, rows) writes NaNs to that token's C outputs (the rule of dvq_embed_gather_f32)
 *   table [rows, C], 16-byte aligned; pos_first, pos_second nullable [C, HW]; h_in [B, C, HW] (NCHW)
 *   C % 4 == 0, C <= 1024, any HW >= 1, any B with B * HW < 2^31 - 64: anything else is DVQ_EINVAL
 * 16-byte loads and stores along the token axis when HW % 4 == 0 and pos_first, pos_second, h_in are 16-byte aligned, 4-byte ones
 * otherwise: the same values.  One launch, no workspace, capturable in a HIP graph.
 */
DVQ_API size_t dvq_decode_table_bytes(int rows, int C);
DVQ_API int dvq_decode_table_prepare_f32(const float *codebook, int rows, int D, const float *conv_weight,
                                         const float *conv_bias, int C, void *table, size_t table_bytes, void *stream);
DVQ_API int dvq_decode_head_f32(const int64_t *codes, int B, int HW, const float *table, int rows, int C,
                                const float *pos_first, const float *pos_second, float *h_in, void *stream);

/*
 * Soft code assignment: distances, soft codes and the code of get_soft_codes in ONE kernel.
 * Replaces: VQEmbedding.compute_distances (quantize2_mask.py:29-48), F.softmax(-distances / temp) and argmin /
 *           torch.multinomial of VectorQuantize2.get_soft_codes (quantize2_mask.py:193-205) and, once per depth,
 *           RQBottleneck.get_soft_codes (quantize_rqvae.py:372-400): four to six passes over a dense [N, K] matrix.
 *   x        [N, D] row-major; codebook [>= K, D], prep from dvq_codebook_prepare_f32 of the SAME K rows
 *   temp     finite, > 0
 *   q        nullable [N, K]: caller-drawn Exp(1) variates (the convention of dvq_sample_head_f32)
 *   soft     nullable [N, K]; dist nullable [N, K]; codes [N] int64
 *   ws       only read when soft == NULL and q != NULL: >= dvq_vq_soft_assign_workspace_bytes(N, D, K) (the scores of the
 *            draw pass through it), 256-byte aligned; NULL / 0 otherwise
 * Per token n:
 *   d[n, j]  = the assign's distance bit for bit: sequential-k fp32 FMA chain, ATen-order norms, fl(fl(xn + en) - 2 dot)
 *   s[n, j]  = (-d[n, j]) / temp (IEEE division, the reference's `-distances / temp`)
 *   soft     = softmax(s) over j: row max, expf, ONE fixed-order sum (accumulated in double), expf / sum -- deterministic:
 *              two runs give the same bits; equal to torch's softmax of the same distances up to expf and summation order
 *   codes[n] = q == NULL: the first-index argmin of d, NaN = minimum -- the code dvq_vq_assign_flat_f32 returns;
 *              q given:   argmax_j soft[n, j] / q[n, j], the first index on ties (what torch.multinomial(soft, 1) computes from
 *                         its own exponential_ draw); a NaN ratio never wins, every ratio NaN gives 0
 * D in {64, 128, 256} (DVQ_EUNSUPPORTED otherwise; other widths by zero padding, as for the assign); K whatever
 * dvq_codebook_prepare_f32 accepts; 1 <= N < 2^31, N * K < 2^40.  DVQ_EINVAL: null x / codebook / prep / codes, temp not
 * finite or <= 0, a missing or too small workspace when one is needed.  Rows are read back with 16-byte accesses when
 * K % 4 == 0 and soft, q, ws are 16-byte aligned, 4-byte ones otherwise: the same values.
 * One launch, no host synchronisation, no allocation: capturable in a HIP graph.  Vector stores only.
 */
DVQ_API size_t dvq_vq_soft_assign_workspace_bytes(int64_t N, int D, int K);
DVQ_API int dvq_vq_soft_assign_flat_f32(const float *x, const float *codebook, const void *prep, int64_t N, int D, int K,
                                        float temp, const float *q, float *soft, float *dist, int64_t *codes,
                                        void *ws, size_t ws_bytes, void *stream);

/*
 * Scored / temperature-sampled code assignment: the learnable-codebook quantizers MaskVectorQuantize / VectorQuantize.
 * Replaces: `dist` (quantize_codebook_mask.py:97-108, quantize.py:92-110) and gumbel_sample(dist, temperature = temp)
 *           (common_utils.py:19-35): the [N, K] score matrix, dist / temp, the uniform noise, two logs, two clamps, an add and
 *           the argmax -- about ten passes over N x K floats; here one sweep that reads u once and writes N codes.
 *   x        [B, D, HW] read in place (NCHW, HW = H*W); HW == 1 is the row-major case [N, D] with B = N
 *   prep     dvq_codebook_prepare_f32 of the codebook the scores are against (for the cosine metrics: of the NORMALISED rows)
 *   metric   DVQ_METRIC_L2:  s = -d, d = the assign's distance bit for bit (sequential-k fp32 FMA chain, ATen-order norms,
 *                            fl(fl(xn + en) - 2 dot)): the reference's -sum x^2 - sum e^2 + 2 x E^T, negation included
 *            DVQ_METRIC_DOT: s = dot, the same chain (use_cosine_sim: the caller passes L2-normalised tokens and rows;
 *                            use_cosine_distance is DVQ_METRIC_L2 on normalised operands)
 *   u        nullable [N, K], N = B * HW: uniforms drawn by the caller, torch.zeros(N, K).uniform_(0, 1) (the reference's own
 *            draw: the generator is consumed identically); u_numel = its element count, checked against N * K
 *   temp     finite, > 0 when u is given; ignored otherwise
 *   codes    [N] int64:
 *            u == NULL: argmax_j s[n, j]
 *            u given:   argmax_j fl(fl(s[n, j] / temp) + g[n, j]),  g = -logf(max(-logf(max(u, 1e-20f)), 1e-20f))
 *            with torch.argmax's rules: the first index among equal maxima; a NaN is the maximum and the first NaN wins
 * D in {64, 128, 256} (DVQ_EUNSUPPORTED otherwise; other widths by zero padding, as for the assign).  DVQ_EINVAL: null x / prep /
 * codes, an unknown metric, u with temp not finite or <= 0, u_numel != N * K.  u is read once, as 16-byte pieces when K % 4 == 0
 * and u is 16-byte aligned, 4-byte ones otherwise: the same values.  Nothing of size N x K is written.
 * One launch, no workspace, no atomics, no host synchronisation: capturable in a HIP graph.  Vector stores only.
 */
#define DVQ_METRIC_L2  0
#define DVQ_METRIC_DOT 1
DVQ_API int dvq_vq_score_assign_f32(const float *x, const void *prep, int B, int D, int HW, int K, int metric, float temp,
                                    const float *u, int64_t u_numel, int64_t *codes, void *stream);

/*
 * Quantisation from GIVEN codes -- the rest of those forwards (quantize_codebook_mask.py:114-121,135; quantize.py:116-119,133):
 * embedding gather, (masked) loss, straight-through add, as one streaming kernel (+ the loss finalize).
 *   z [B, D, HW] (flat: [N, D]); codes [B, HW] int64 (a code outside [0, K): z_q = z, no loss term); codebook [>= K, D], 16-byte
 *   aligned; mask nullable [B, HW]; zq nullable [B, D, HW] = fl(z + fl(e - z)); loss nullable [2]: loss[0] = mean((e - z)^2 * mask),
 *   loss[1] = fl(fl(beta * mean) + mean) (partials in double, summed in one fixed order);
 *   ws: only when loss is wanted, >= dvq_vq_assign_workspace_bytes(B, D, HW, K, DVQ_MODE_EXACT), 256-byte aligned.
 * Fed the codes dvq_vq_assign_nchw_f32 returns, zq is bit-identical to that op's and the loss agrees within 1e-5 relative.
 * D a multiple of 16.
 */
DVQ_API int dvq_vq_apply_codes_nchw_f32(const float *z, const int64_t *codes, const float *codebook, const float *mask,
                                        int B, int D, int HW, int K, float beta, float *zq, float *loss,
                                        void *ws, size_t ws_bytes, void *stream);
DVQ_API int dvq_vq_apply_codes_flat_f32(const float *z, const int64_t *codes, const float *codebook, const float *mask,
                                        int64_t N, int D, int K, float beta, float *zq, float *loss,
                                        void *ws, size_t ws_bytes, void *stream);

/*
 * GumbelQuantize (hard / straight-through forward): projection to K logits, Gumbel-max code, KL term and z_q in ONE sweep.
 * Replaces: GumbelQuantize.forward (quantize_vqgan.py:171-200): the 1x1 `proj` conv, F.gumbel_softmax (the Exp(1) draw's log,
 *           the add, the divide by tau, a softmax, the hard one-hot), the dense [N, K] x [K, d] einsum with a one-hot left operand,
 *           a second softmax and a log for the KL term, an argmax -- about ten passes over [N, K] floats.  Here z and q are read
 *           once; N codes, one scalar and z_q are written; nothing of size N x K is.
 *
 * dvq_gumbel_prepare_f32 -- once per (proj.weight, proj.bias): the codebook prep's f32 tile images of weight [K, C] (built by
 *   the same kernel dvq_codebook_prepare_f32 runs), with bias [K] (nullable: zeros) where the images carry the row norms.
 *   prep: >= dvq_gumbel_prep_bytes(K, C) (0: unsupported shape), 256-byte aligned.  Only dvq_vq_gumbel_assign_f32 reads it.
 *
 * dvq_vq_gumbel_assign_f32
 *   z      [B, C, HW] read in place (NCHW); HW == 1 is the flat case [N, C] with B = N
 *   embed  [K, d] row-major, d any positive value (read with 16-byte loads when d % 8 == 0 and embed is 16-byte aligned)
 *   q      nullable [B, K, HW]: the Exp(1) variates F.gumbel_softmax draws (-empty_like(logits).exponential_().log()), drawn by
 *          the caller in the logits' own layout -- torch's generator is consumed as in the reference
 *   tau    finite, > 0 when q is given; ignored otherwise
 *   kl_K   the factor inside the KL term's log (the module passes n_embed); finite, > 0
 *   zq     nullable [B, d, HW]; codes [B, HW] int64; kl nullable [1]
 *   ws     only when kl is wanted: >= dvq_vq_gumbel_assign_workspace_bytes(B, HW), 256-byte aligned
 * Per token n:
 *   l_k      = fl(dot(z_n, W_k) + b_k): the sequential-k fp32 FMA chain of dvq_vq_score_assign_f32, the bias added after it
 *   codes[n] = q == NULL: argmax_k l_k;  q given: argmax_k fl(fl(l_k + g_k) / tau), g_k = -logf(q_k)
 *              with torch.argmax's rules: the first index among equal maxima; a NaN is the maximum and the first NaN wins
 *   KL_n     = sum_k p_k log(p_k kl_K + 1e-10), p = softmax(l), evaluated online as A / S - m - log S + log kl_K with the
 *              running maximum m, S = sum e^(l - m), A = sum e^(l - m) l -- WITHOUT the 1e-10: each term differs by
 *              p log(1 + 1e-10 / (p kl_K)) <= 1e-10 / kl_K, the sum by at most 1e-10 K / kl_K, i.e. 1e-10 per token when
 *              kl_K = K, against KL values of order 0.01 to 10
 *   kl[0]    = mean_n KL_n: one double partial per workgroup, added in one fixed order by a finalize kernel -- deterministic
 *   zq[b, :, hw] = embed[codes[n], :], the codebook row ITSELF (bit-equal).  The reference's value is f embed[code] with
 *              f = fl(fl(1 - y) + y), y the winner's soft probability in (0, 1]: |f - 1| <= 2^-23
 * C in {64, 128, 256}: DVQ_EUNSUPPORTED otherwise.  DVQ_EINVAL: null z / prep / embed / codes, tau not finite or <= 0 when q is
 * given, kl_K <= 0, a missing or too small workspace when kl is wanted, a misaligned pointer.  B * HW < 2^31.
 * Two launches (the sweep, the finalize when kl is wanted) on one stream: no atomics, no host synchronisation, no allocation;
 * capturable in a HIP graph as a single chain.  Vector stores only.
 */
DVQ_API size_t dvq_gumbel_prep_bytes(int K, int C);
DVQ_API int dvq_gumbel_prepare_f32(const float *weight, const float *bias, int K, int C, void *prep, size_t prep_bytes,
                                   void *stream);
DVQ_API size_t dvq_vq_gumbel_assign_workspace_bytes(int B, int HW);
DVQ_API int dvq_vq_gumbel_assign_f32(const float *z, const void *prep, const float *embed, int B, int C, int HW, int K, int d,
                                     float tau, float kl_K, const float *q, float *zq, int64_t *codes, float *kl,
                                     void *ws, size_t ws_bytes, void *stream);

/*
 * GumbelQuantize, the training step of the hard (straight-through) form: a forward that keeps the logits, and the backward down to them.
 * Replaces: what autograd records for GumbelQuantize.forward (quantize_vqgan.py:171-200) and replays backwards -- the one-hot einsum,
 *           F.gumbel_softmax's softmax and divide, the second softmax, log and sum of the KL term: ten passes over [N, K] floats and
 *           their saved [N, K] tensors, and as many again.  Here one [N, K] tensor (the logits) is saved next to the variates q.
 *
 * dvq_vq_gumbel_forward_train_f32 -- dvq_vq_gumbel_assign_f32 with one more output:
 *   logits [B, K, HW] (the layout of q), not null: l_k as defined there, bit for bit what the sweep compares.  Every other argument, the
 *   prep image (dvq_gumbel_prepare_f32), the workspace (dvq_vq_gumbel_assign_workspace_bytes), the checks and their words are that
 *   entry point's; codes, zq and kl are its bits.  DVQ_EINVAL also for a null or misaligned logits.
 *
 * dvq_vq_gumbel_backward_f32 -- dlogits [B, K, HW] from the saved logits; per token n, N = B HW:
 *   s_k  = fl(fl(l_k - logf(q_k)) / tau)  (q == NULL: fl(l_k / tau)): the forward's operations in the forward's order
 *   y    = softmax(s), p = softmax(l), delta = sum_k y_k u_k, KL_n = sum_k p_k log(p_k kl_K)
 *   dl_k = y_k (u_k - delta) / tau  +  (g_kl[0] / N) p_k (log p_k + log kl_K - KL_n)
 *   logits [B, K, HW]; q nullable [B, K, HW], the forward's variates (not read when u is NULL)
 *   u      nullable [B, K, HW]: u[b, k, hw] = embed[k, :] . G[b, :, hw], G = dL/dz_q -- the hard form's straight-through gradient, a GEMM
 *          the caller makes; NULL: no gradient arrives through z_q and the first term is left out
 *   g_kl   nullable, a DEVICE pointer to one float, dL/dkl of the forward's kl[0] (the mean over tokens); NULL: the second term is left out.
 *          u and g_kl both NULL: dlogits is zero-filled
 *   tau    finite, > 0 when u is given;  kl_K finite, > 0 when g_kl is given (the value cancels: log kl_K stands in KL_n as well)
 *   dlogits may be u itself (the same lane reads u_k and then writes dl_k over it), and nothing else: its B K HW floats may not
 *          overlap logits, q or g_kl anywhere, nor u at an offset (DVQ_EINVAL: the ranges are compared, not only the pointers)
 *   ws, ws_bytes: reserved, not read (pass NULL, 0): the kernel keeps its partial sums in LDS
 *   A term with p_k == 0 is 0 (a code whose logit is -inf gets exactly 0, as torch gives).  A token whose logits are all -inf, or hold a
 *   NaN, has NaN in every dl_k, as the torch chain has.
 * DVQ_EINVAL: null logits / dlogits, a non-positive size, tau / kl_K as above, a misaligned pointer, dlogits overlapping logits, q, g_kl, or u other than as a whole.
 * DVQ_EUNSUPPORTED: B * HW >= 2^31 or B * HW * K >= 2^40.  Any K.  One launch, no atomics, no host synchronisation, no allocation;
 * vector stores only; the same bits run to run.  dW, db, dz are GEMMs of the caller on dlogits; dembed is dvq_code_sums_det /
 * dvq_ema_accumulate_nchw_f32 of G under the forward's codes.
 */
DVQ_API int dvq_vq_gumbel_forward_train_f32(const float *z, const void *prep, const float *embed, int B, int C, int HW, int K, int d,
                                            float tau, float kl_K, const float *q, float *zq, int64_t *codes, float *kl,
                                            float *logits, void *ws, size_t ws_bytes, void *stream);
DVQ_API int dvq_vq_gumbel_backward_f32(const float *logits, const float *q, const float *u, const float *g_kl, int B, int HW, int K,
                                       float tau, float kl_K, float *dlogits, void *ws, size_t ws_bytes, void *stream);

/*
 * Nearest-codebook assignment at the NARROW widths D = 4, 8, 16: codes, z_q and the commitment loss in one exact kernel.
 * Replaces: the same reference ops as dvq_vq_assign_nchw_f32 / dvq_vq_assign_flat_f32 -- VectorQuantize2.forward
 *           (quantize2_mask.py:157-191 around VQEmbedding.compute_distances :29-48, find_nearest_embedding :50-55, embed :130-132)
 *           and VectorQuantizer2.forward (quantize_vqgan.py:271-312) -- for taming-style checkpoints (embed_dim 3 or 4,
 *           K = 8192 / 16384) and factorised low-dimensional codebooks.  No prepared codebook image: the kernel stages the
 *           codebook rows itself and computes their norms while it does.
 *   z        _nchw: [B, D, HW] read in place, any HW, 4-byte aligned;  _flat: row-major [N, D], 16-byte aligned
 *   codebook [K, D], 16-byte aligned (for VQEmbedding pass weight[:-1])
 *   mask     nullable [B, HW] / [N]
 *   zq       nullable, the layout (and, _flat, the alignment) of z:  fl(z + fl(e - z))
 *   codes    [B, HW] / [N] int64: first-index argmin, NaN = minimum (torch CPU semantics)
 *   loss     nullable [2] f32: loss[0] = mean((e-z)^2*mask), loss[1] = fl(fl(beta*mean)+mean)
 *   ws       only when loss is wanted: >= dvq_vq_assign_narrow_workspace_bytes(N) (N = B * HW; 0 for N <= 0), 256-byte aligned
 * Every (token, code) distance is the reference's fp32 arithmetic bit for bit: acc = fma(z[k], e[k], acc) for k ascending from 0,
 * d = fl(fl(xn + en) - 2 acc), with xn / en = torch-CPU's sum of squares at these widths (D <= 8: the sequential sum of the
 * rounded squares; D = 16: t[l] = sq[l] + sq[l + 8], then t[0] + ... + t[7] left to right) -- pinned on the reference by
 * tests/golden/narrow_D*.npz.  D = 3: append one zero channel to latents and codebook and run at 4 (exact: fma(0, 0, acc) = acc,
 * + 0 in the norm); multiply loss[0] by 4 / 3.  The Python drop-in does this.
 * The codebook is walked in LDS tiles of dvq_vq_assign_narrow_tile_codes(D) codes (0 for an unsupported D); K need not be a
 * multiple.  Every workgroup walks the whole codebook for its tokens: 256 tokens per workgroup, 64 up to DVQ_NARROW_SMALL_N tokens
 * (same arithmetic, same results; a small batch fills more of the chip).  K < 2^20, N < 2^31: DVQ_EUNSUPPORTED beyond, as is D outside {4, 8, 16}.  DVQ_EINVAL: null z / codebook / codes, a
 * non-positive size, a misaligned pointer, a missing or too small workspace when loss is wanted.
 * Two launches (the assign, the loss finalize when loss is wanted) on one stream: one double partial per workgroup added in a
 * fixed order -- no atomics, the same bits every run; no host synchronisation, no allocation.  Vector stores only.
 */
#define DVQ_NARROW_SMALL_N 65536    /* up to this many tokens: 64 per workgroup (one wave); above: 256 (two waves, two tokens per lane) */
DVQ_API size_t dvq_vq_assign_narrow_workspace_bytes(int64_t N);
DVQ_API int dvq_vq_assign_narrow_tile_codes(int D);
DVQ_API int dvq_vq_assign_narrow_nchw_f32(const float *z, const float *codebook, const float *mask, int B, int D, int HW, int K,
                                          float beta, float *zq, int64_t *codes, float *loss, void *ws, size_t ws_bytes,
                                          void *stream);
DVQ_API int dvq_vq_assign_narrow_flat_f32(const float *z, const float *codebook, const float *mask, int64_t N, int D, int K,
                                          float beta, float *zq, int64_t *codes, float *loss, void *ws, size_t ws_bytes,
                                          void *stream);

/*
 * Wire format of the image-parallel exchange (one all-gather per batch; the reference gathers nothing --
 * it runs one process per GPU under Lightning DDP, train.py:230 -- this is what lets downstream consumers
 * (permuter, stage-2 transformer) see the global code tensor).  Per rank one byte buffer of
 * dvq_exchange_bytes(): [codes as int16 (num_codes <= 32768) / int32, b_max images][grain indices as int8]
 * [(loss numerator, element count) as 2 x float64]; the first two sections are zero padded to a multiple of
 * 8 bytes, and pack writes every byte of the buffer.
 *   pack    codes [b_local, codes_per_image] int64, grain [b_local, grain_per_image] int64 (nullable when
 *           grain_per_image == 0), loss nullable ([0] = local mean; numel = local element count; the pair is
 *           (0, 0) without a loss or with numel == 0); rows b_local .. b_max-1 are zero padding (ragged
 *           shards); an empty shard (b_local == 0) may pass null codes and grain; buf 8-byte aligned
 *   unpack  gathered [world, bytes], 8-byte aligned -> codes [global_batch, codes_per_image] int64, grain, mean[0] = global
 *           mean (pairs added in rank order: same bits on every rank); shard r holds the images
 *           [r*base + min(r, extra), ...) of global_batch = world*base + extra, b_max = ceil(global_batch / world)
 */
DVQ_API size_t dvq_exchange_bytes(int64_t codes_per_image, int64_t grain_per_image, int b_max, int num_codes);
DVQ_API int dvq_exchange_pack(const int64_t *codes, const int64_t *grain, const float *loss, double numel, int b_local,
                      int b_max, int64_t codes_per_image, int64_t grain_per_image, int num_codes, void *buf,
                      void *stream);
DVQ_API int dvq_exchange_unpack(const void *gathered, int world, int global_batch, int64_t codes_per_image,
                        int64_t grain_per_image, int num_codes, int64_t *codes, int64_t *grain, float *mean,
                        void *stream);

/*
 * Temperature-sampled code assignment against -cdist: EuclideanCodebook with sample_codebook_temp > 0
 * (quantize_lucidrains.py:123-125: `dist = -torch.cdist(flatten, embed)`, gumbel_sample(dist, temperature = temp)).
 * dvq_vq_score_assign_f32 with a third score: s = -sqrtf(d < 0 ? 0 : d), d = the assign's distance bit for bit (a NaN d stays a
 * NaN score: the maximum); the square root does not commute with the noise, so DVQ_METRIC_L2 cannot serve this codebook.
 *   codes [N] int64 = argmax_j fl(fl(s[n, j] / temp) + g[n, j]), g and the argmax rules as dvq_vq_score_assign_f32
 * x, prep, B, D, HW, K, u, u_numel as there; u is REQUIRED (temp == 0 is the plain assign) and temp finite, > 0.
 * DVQ_EINVAL: null x / prep / u / codes, sizes, temp, u_numel != N * K, misaligned pointers.  DVQ_EUNSUPPORTED: D outside {64, 128, 256},
 * tensor too large.  One launch, no N x K store, no workspace, no atomics, no host synchronisation.  Vector stores only.
 */
DVQ_API int dvq_vq_cdist_sample_assign_f32(const float *x, const void *prep, int B, int D, int HW, int K, float temp,
                                           const float *u, int64_t u_numel, int64_t *codes, void *stream);

/*
 * Orthogonal regulariser of a codebook, eq. (2) of arXiv 2112.00384 (quantize_lucidrains.py:18-24, orthogonal_loss_fn; the same
 * expression sits in quantize_codebook_mask.py:124-132 and quantize.py), and its gradient (ortho_loss.hip).
 *   t [h, n, d] f32, 16-byte aligned; c^_i = t_i / max(|t_i|, 1e-12) (F.normalize); C = c^ c^T per head
 *   forward:  rinv [h, n] = 1 / max(|t_i|, 1e-12) (written; keep it for backward), loss [1] = sum (C - I)^2 / (h n^2)
 *             ws >= dvq_ortho_loss_workspace_bytes(h, n, d), 256-byte aligned (forward: one double per workgroup; backward: the
 *             partial gradients of the up to 8 column slices its sweep is split into, at most 8 h n d floats)
 *   backward: grad [h, n, d] = grad_out[0] * dloss/dt (grad_out: a DEVICE scalar), every element written once; must not alias t;
 *             ws as for forward (its contents need not survive from forward)
 * The Gram matrix is tiled over its upper triangle on the fp32 MFMA chains of the assign; nothing of size n x n reaches memory, no
 * float atomics; partial sums in double, finalised in one fixed order: loss and grad are the same bits on every run.  Within 1e-5
 * relative of the float64 value.  No host synchronisation; capturable in a HIP graph.
 * d in {64, 128, 256}, h < 2^16, n < 2^24: DVQ_EUNSUPPORTED otherwise (dvq_ortho_loss_workspace_bytes: 0).  DVQ_EINVAL: null pointer,
 * h or n < 1, misaligned pointer, grad == t.  DVQ_EWORKSPACE: ws too small.
 */
DVQ_API size_t dvq_ortho_loss_workspace_bytes(int h, int n, int d);
DVQ_API int dvq_ortho_loss_forward_f32(const float *t, int h, int n, int d, float *rinv, float *loss, void *ws, size_t ws_bytes,
                                       void *stream);
DVQ_API int dvq_ortho_loss_backward_f32(const float *t, const float *rinv, const float *grad_out, int h, int n, int d, float *grad,
                                        void *ws, size_t ws_bytes, void *stream);

/*
 * The training-mode codebook update of EuclideanCodebook (kind 0, quantize_lucidrains.py:131-144) and CosineSimCodebook (kind 1,
 * :257-279) as ONE launch, code expiry included (:85-105):
 *   both    cluster_size_out = cluster_size * decay + (1 - decay) * counts       (counts [K] f32: this step's tokens per code)
 *   kind 0  embed = embed_avg / (((cluster_size_out + eps) / (S + K eps)) * S), S = sum of cluster_size_out (in double).  embed_avg
 *           [K, D] is only read: the reference never updates it.  sums is ignored (may be NULL).
 *   kind 1  sums [K, D] = per-code sums of the L2-normalised tokens (dvq_ema_accumulate_nchw_f32 on the normalised rows):
 *           m = normalize(sums / max(counts, 1)), a code without tokens takes normalize(embed) instead;
 *           embed = embed * decay + (1 - decay) * m.  embed_avg is ignored (may be NULL).
 *   expiry  pick != NULL and threshold > 0: the j-th code (in index order) with cluster_size_out < threshold takes token pick[j] of x
 *           -- [B, D, HW] (NCHW), HW == 1: row-major [N, D] with B = N -- L2-normalised (in BOTH kinds, as the reference does).
 *           pick [K] int64 in [0, B * HW) (dvq_restart_pick_i64: distinct, no host read; values outside are clamped).
 * cluster_size_out must not alias cluster_size; embed [K, D] is updated in place (a row has one owner).  `1 - decay` as
 * dvq_ema_update_f32: the Python double, rounded to fp32.  Within rounding (1e-5) of the reference.  No atomics, no host
 * synchronisation.  DVQ_EINVAL: kind not 0 / 1, null pointer, K or D < 1, aliasing, decay outside [0, 1], threshold < 0, pick without x.
 */
DVQ_API int dvq_lucid_update_f32(int kind, const float *counts, const float *sums, float decay, float eps, float threshold,
                                 int K, int D, const float *cluster_size, float *cluster_size_out, const float *embed_avg,
                                 float *embed, const float *x, int B, int HW, const int64_t *pick, void *stream);

/*
 * 16-bit latents: the dense assign, its backward and the EMA statistics on fp16 / bf16 tensors (an encoder trunk run under autocast
 * hands the quantizer such latents; casting them to float32 and z_q back costs two extra passes over [B, D, H, W]).
 * Only LATENT-SHAPED tensors change type: z, zq, g_zq, g_z are `dtype` (DVQ_DTYPE_F16: IEEE binary16; DVQ_DTYPE_BF16: bfloat16),
 * 2-byte aligned; the codebook, prep buffer, mask, loss, statistics and g_loss stay float32.  With zf = float32(z) (exact; fp16
 * subnormals included):
 *   dvq_vq_assign_nchw_x16     codes: bit for bit those of dvq_vq_assign_nchw_f32 on zf (first-index / NaN rules included);
 *                              loss[0..1]: that op's on zf, from fp32 (e - zf) before any narrowing (1e-5 relative);
 *                              zq = narrow(fl(zf + fl(e - zf))): the fp32 op's value rounded ONCE to `dtype`, to nearest even (the bits
 *                              of torch's zq_f32.to(dtype); NaN stays NaN, payload unspecified; fp16 overflow gives +-inf).
 *                              z / zq [B, D, HW] of `dtype` (HW == 1: row-major [N, D], B = N); zq nullable.  prep: the unchanged
 *                              dvq_codebook_prepare_f32 buffer.  ws >= dvq_vq_assign_workspace_bytes(B, D, HW, K, mode), the layout
 *                              group is "dense" (DVQ_MODE_WS_CLEAN is honoured, also between this op and dvq_vq_assign_nchw_f32 of the
 *                              same shape); dvq_vq_assign_fallback_count_offset applies.  mode: DVQ_MODE_FILTER or DVQ_MODE_EXACT
 *                              (DVQ_MODE_FILTER_PASS1 / DVQ_MODE_FILTER_WIDE: DVQ_EUNSUPPORTED).  D in {64, 128, 256}; the narrow widths
 *                              (3, 4, 8, 16) and every other D: DVQ_EUNSUPPORTED.  Pass 1 runs the lane-per-token form for every shape
 *                              (no split / wide / row-major form: a small batch runs unsplit).
 *                              DVQ_EINVAL: dtype not 1 / 2; null z / codebook / prep / codes; z or zq not 2-byte aligned; the size rules of
 *                              the f32 op.  DVQ_EWORKSPACE: ws too small.
 *   dvq_vq_backward_nchw_x16   g_z = narrow(g_zq_f + (g_loss * coef_scale) * ((zf - e) * m)), the fp32 operation order of
 *                              dvq_vq_backward_nchw_f32 on the widened inputs, narrowed once.  z, g_zq (nullable), g_z of `dtype`;
 *                              g_loss (nullable, not both) a float32 device scalar; argument rules as the f32 op.
 *   dvq_ema_accumulate_nchw_x16  cluster_size / vectors_sum over zf, float32, accumulated as dvq_ema_accumulate_nchw_f32 does (float
 *                              atomics: equal to rounding, 1e-5).  Any 2-byte aligned z, any HW.
 * Vector and buffer stores only.  dvq_ema_update_f32 has no 16-bit twin: pass restart = 1 with the K restart rows gathered and widened.
 */
#define DVQ_DTYPE_F16 1   // IEEE binary16
#define DVQ_DTYPE_BF16 2  // bfloat16: the upper 16 bits of a float32
DVQ_API int dvq_vq_assign_nchw_x16(const void *z, int dtype, const float *codebook, const void *prep, const float *mask,
                                   int B, int D, int HW, int K, float beta, void *zq, int64_t *codes, float *loss,
                                   void *ws, size_t ws_bytes, int mode, void *stream);
DVQ_API int dvq_vq_backward_nchw_x16(const void *z, int dtype, const float *codebook, const int64_t *codes, const float *mask,
                                     const void *g_zq, const float *g_loss, float coef_scale, int B, int D, int HW, int K,
                                     void *g_z, void *stream);
DVQ_API int dvq_ema_accumulate_nchw_x16(const void *z, int dtype, const int64_t *codes, int B, int D, int HW, int K,
                                        float *cluster_size, float *vectors_sum, void *stream);

/*
 * BIT-REPRODUCIBLE per-code sums: the statistics of dvq_ema_accumulate_nchw_f32 / _x16 and the gradient of
 * dvq_vq_backward_codebook_nchw_f32 in ONE FIXED summation order -- no float atomic and no rank taken from a returning atomic on the
 * path, so two calls on equal inputs give equal bits, whatever the grid, the occupancy or the timing.
 * Tokens are numbered n = b * HW + hw (HW == 1: n = the row of a row-major z [N, D], B = N); v[n][c] is the token's fp32 value at
 * channel c -- float32(z) for the statistics (exact for DVQ_DTYPE_F16 / DVQ_DTYPE_BF16), fl(fl(z - codebook[j][c]) * mask[n]) with
 * j = codes[n] for the gradient (mask == NULL: 1).  Codes outside [0, K) are ignored.  For every code j and channel c:
 *   1. the tokens are cut into tiles of DVQ_DET_TILE = 2048 consecutive n (tile i holds n in [2048 i, 2048 i + 2048));
 *   2. inside a tile the members of j (tokens with codes[n] == j) are taken in ascending n and cut into runs of DVQ_DET_RUN = 32 members
 *      (the last run of a tile may be shorter);
 *   3. a run's sum is r = v[first member]; r = fl(r + v[next member]) ... in that order;
 *   4. the tile's partial is p = r_0; p = fl(p + r_1); ... over its runs in order;
 *   5. S[j][c] = p of the first tile that has a member of j; S = fl(S + p of the next such tile) ... in ascending tile index.
 *      A code without members has S = +0.0f.
 * The order is a function of (v, codes, N, D, K) only: not of the B x HW factorisation, the layout (NCHW or row-major), the storage
 * type beyond the widening, or the alignment of z (which only select how values are loaded).
 *   dvq_code_sums_det                  cluster_size[j] = the member count (exact below 2^24), vectors_sum[j][c] = S[j][c]; both overwritten.
 *                                      dtype 0 (float32), DVQ_DTYPE_F16, DVQ_DTYPE_BF16; z [B, D, HW] of that type.
 *   dvq_vq_backward_codebook_det_f32   g_weight[j][c] = fl(k * S[j][c]) with k = -fl(g_loss[0] * coef_scale), WRITTEN (not accumulated) for
 *                                      rows 0 .. K - 1 (a row without members: k * 0); arguments as dvq_vq_backward_codebook_nchw_f32.
 * D % 4 == 0 and K <= DVQ_DET_MAX_K = 16384 (DVQ_EUNSUPPORTED otherwise; the message names the limit), B * HW < 2^31.  ws: caller-provided,
 * 256-byte aligned, at least the *_workspace_bytes of the same (B, D, HW, K) -- (B HW / 2048 tiles) x (min(K, 2048) rows of D floats, plus
 * 2 K + 12 KiB of tables); contents need not be kept or cleared between calls.  The query returns 0 for a shape the call refuses.
 * Three launches on `stream`, no host synchronisation, capturable in a graph.  DVQ_EINVAL: null pointer (mask is nullable), dtype not
 * 0 / 1 / 2, a size <= 0, z not aligned to its element, vectors_sum / g_weight / codebook not 16-byte aligned, ws not 256-byte aligned.
 * DVQ_EWORKSPACE: ws null or too small.  No atomics: a partial row leaves as 4-byte vector stores, sixteen
 * lanes writing 64 contiguous bytes; the results as 16-byte stores.
 */
enum { DVQ_DET_TILE = 2048, DVQ_DET_RUN = 32, DVQ_DET_MAX_K = 16384 };
DVQ_API size_t dvq_code_sums_det_workspace_bytes(int B, int D, int HW, int K);
DVQ_API int dvq_code_sums_det(const void *z, int dtype, const int64_t *codes, int B, int D, int HW, int K, float *cluster_size,
                              float *vectors_sum, void *ws, size_t ws_bytes, void *stream);
DVQ_API size_t dvq_vq_backward_codebook_det_workspace_bytes(int B, int D, int HW, int K);
DVQ_API int dvq_vq_backward_codebook_det_f32(const float *z, const float *codebook, const int64_t *codes, const float *mask,
                                             const float *g_loss, float coef_scale, int B, int D, int HW, int K, float *g_weight,
                                             void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DVQ_H_ */
