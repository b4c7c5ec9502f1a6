// launchers.h -- every host function that one unit of libdvq.so defines and another calls, declared once: the launchers next to
// their kernels, and the size / grid helpers the C ABI layer (dvq_abi.hip) asks them for.  The defining unit and every caller
// include this header, so a definition that drifts from its declaration fails to compile (return type) or to link (parameter
// list: -Wl,--no-undefined).  Default arguments live here only.  The per-width pass-1 launchers and the resolver: dvq_pass1.h.
#pragma once
#include "dvq_filter.h"

int dvq_prep_codes_per_workgroup(int K);
int dvq_launch_prep_f32(const float *E, int K, int D, void *prep, hipStream_t st);
int dvq_launch_prep_f16(const float *E, int K, int D, void *prep, hipStream_t st);
int dvq_launch_exact(const float *z, const float *prep, const float *E, const float *mask,
                     int D, int HW, int K, long N, float *zq, long long *codes, double *partials,
                     const DvqRouted *rv, hipStream_t st, int xt = 0);
int dvq_launch_filter(const float *z, const void *prep, const float *E, const float *mask,
                      int D, int HW, int K, long N, float *zq, long long *codes, double *partials,
                      void *ws_extra, bool pass1_only, bool force_wide, float *loss, float beta,
                      const DvqRouted *rv, hipStream_t st, const DvqConv *cv, const DvqFold *fd, bool ws_clean, int xt = 0);
int dvq_launch_exact_list(const float *z, const float *prep, const float *E, const float *mask,
                          int D, int HW, int K, long N, float *zq, long long *codes, double *partials,
                          const int *list, const int *list_count, DvqLossTail tail, const DvqRouted *rv,
                          hipStream_t st, const DvqConv *fold_conv = nullptr, int xt = 0);
int dvq_launch_routed_prepass(int G, int gate_mode, const void *gate, float thr, int B, int hc, int wc,
                              long long *indices, float *cmask, long long *gate_out, hipStream_t st);
int dvq_launch_routed(int G, int gate_mode, const void *gate, float thr, const float *h_coarse,
                      const float *h_median, const float *h_fine, const void *prep, const float *E,
                      int B, int D, int hc, int wc, int K, float beta, float *zq, long long *codes,
                      float *loss, long long *indices, float *cmask, long long *gate_out,
                      double *partials, void *ws_extra, bool exact, bool pass1_only, hipStream_t st, const DvqConv *cv,
                      const DvqFold *fd, bool ws_clean);
size_t dvq_fold_prep_bytes_impl(int K, int D);
int dvq_launch_fold_prep(const float *E, int K, int D, const void *cbprep, const float *Wt, const float *bias, void *fprep,
                         hipStream_t st);
size_t dvq_filter_ws_extra_bytes(int D, int HW, int K, long N);
bool dvq_filter_supported(int D, int HW, int K, long N);
int dvq_launch_loss_finalize(const double *partials, int nparts, double inv_numel, float beta,
                             float *loss, hipStream_t st);
int dvq_launch_route_select(int G, int gate_mode, const void *gate, const float *h_coarse,
                            const float *h_median, const float *h_fine, int B, int C, int hc, int wc,
                            float *h_out, long long *indices, float *cmask, float thr, long long *gate_out,
                            hipStream_t st);
// the select on 2-byte features (fp16 or bf16: nothing is converted); gate_mode 0 / 1 only
int dvq_launch_route_select_x16(int G, int gate_mode, const void *gate, const void *h_coarse, const void *h_median,
                                const void *h_fine, int B, int C, int hc, int wc, void *h_out, long long *indices,
                                float *cmask, hipStream_t st);
// the select on channels_last features (DVQ_NHWC: [B, rows, cols, C]) of es-byte elements, moved as bytes; gate_mode 0 / 1 only
int dvq_launch_route_select_rows(int G, int gate_mode, const void *gate, const void *h_coarse, const void *h_median,
                                 const void *h_fine, int es, int B, int C, int hc, int wc, void *h_out, long long *indices,
                                 float *cmask, hipStream_t st);
int dvq_launch_entropy_gate(const float *ent, long n, float thr, long long *gate, hipStream_t st);
// xt (here and below): the type of the latent-shaped tensors, 0 = float32, DVQ_DTYPE_F16 / DVQ_DTYPE_BF16 (dvq_common.h: DvqLat);
// anything else returns -1000
int dvq_launch_vq_backward_z(const void *z, int xt, const float *E, const long long *codes, const float *mask, const void *g_zq,
                             const float *g_loss, float coef_scale, int D, int HW, int K, long N, void *gz, hipStream_t st);
int dvq_launch_ema_accumulate(const void *z, int xt, const long long *codes, int D, int HW, long N, int K,
                              float *cluster_size, float *vectors_sum, hipStream_t st);
int dvq_launch_codebook_grad(const float *z, const float *E, const long long *codes, const float *mask, const float *g_loss,
                             float coef_scale, int D, int HW, long N, int K, float *gw, hipStream_t st);
// the same three for row-major latents [N, D] (train_rows.hip; a channels_last image map is such a matrix): the backward reads
// 16-byte pieces of a row (D % 16 == 0, 16-byte aligned z, g_zq, gz, E), the two sums read per element and have no limit on K;
// the C ABI picks them for HW == 1
int dvq_launch_vq_backward_rows(const void *z, int xt, const float *E, const long long *codes, const float *mask, const void *g_zq,
                                const float *g_loss, float coef_scale, int D, int K, long N, void *gz, hipStream_t st);
int dvq_launch_ema_accumulate_rows(const void *z, int xt, const long long *codes, int D, long N, int K, float *cluster_size,
                                   float *vectors_sum, hipStream_t st);
int dvq_launch_codebook_grad_rows(const float *z, const float *E, const long long *codes, const float *mask, const float *g_loss,
                                  float coef_scale, int D, long N, int K, float *gw, hipStream_t st);
int dvq_launch_ema_zero(float *a, size_t na, float *b, size_t nb, hipStream_t st);
int dvq_launch_ema_accumulate_sorted_rows(const float *z, const long long *codes, int D, long N, int K, float *cluster_size,
                                          float *vectors_sum, hipStream_t st);   // -1: not its shape, nothing launched
// the same sums in one fixed summation order (code_sums_det.hip; include/dvq.h: dvq_code_sums_det): E == nullptr the statistics, else
// the codebook gradient (float32 z); no float atomics; ws of dvq_code_sums_det_ws_bytes(N, D, K) bytes; D % 4 == 0, K <= 16384, N < 2^31
size_t dvq_code_sums_det_ws_bytes(long N, int D, int K);
int dvq_launch_code_sums_det(const void *z, int xt, const float *E, const long long *codes, const float *mask, const float *g_loss,
                             float coef_scale, int D, int HW, long N, int K, float *count, float *out, void *ws, hipStream_t st);
int dvq_launch_embed_gather(const float *E, int K, int D, const long long *idx, long n, float *out,
                            hipStream_t st);

int dvq_launch_permute_count(const long long *grain, int B, int ncell, int *counts, int *maxes, hipStream_t st);
int dvq_launch_permute_forward(const long long *codes, const long long *grain, int B, int hc, int wc,
                               int row_first, int Lc, int Lf, const long long *special,
                               long long *cc, long long *cp, long long *cs, long long *fc, long long *fp,
                               long long *fs, hipStream_t st);
int dvq_launch_permute_backward(const long long *cc, const long long *fc, const long long *cp,
                                const long long *fp, int B, int Lc, int Lf, int hc, int wc,
                                long long cpos_eos, long long fpos_eos, long long *target, hipStream_t st);
int dvq_permute_max_cells(void);
int dvq_launch_sample_head(const float *logits, long long lstride, int B, int V, float temperature, const long long *rules,
                           const long long *hist, long long hstride, int hlen, float *flag, int top_k, float top_p,
                           int sample, const float *q, long long *tokens, long long tstride, float *out_logits,
                           float *out_probs, hipStream_t st);
int dvq_launch_transfer_count(const long long *cp, long long cstride, int B, int Lc, int hc, long long ceos, int remain,
                              int *counts, int *maxes, hipStream_t st);
int dvq_launch_transfer_fill(const long long *cp, long long cstride, int B, int Lc, int hc, long long ceos, int remain,
                             int row_first, int sos_mode, long long sos, long long feos, long long fpad, int L, long long *out,
                             hipStream_t st);
int dvq_sample_max_vocab(void);
int dvq_sample_max_cells(void);
int dvq_launch_decode_table(const float *E, int rows, int D, const float *W, const float *bias, int C, float *T, hipStream_t st);
int dvq_launch_decode_head(const long long *codes, int B, int HW, const float *T, int rows, int C, const float *F, const float *L,
                           float *out, hipStream_t st);
int dvq_launch_code_stats(const long long *codes, long N, int K, long long *counts, long long *n_used, float *perplexity,
                          float *onehot, hipStream_t st);
int dvq_launch_code_stats_grain(const long long *codes, const long long *grain, int B, int H, int W, int hc, int wc, int G, int K,
                                long long *counts, long long *n_tokens, long long *n_used, float *perplexity, hipStream_t st);
int dvq_launch_entropy_map(const float *img, int B, int H, int W, float *out, hipStream_t st);
size_t dvq_router_gate_ws_bytes(int nb, int B, int C, int hc, int wc, int groups, int Hid);
size_t dvq_router_gate_prep_bytes_impl(int nb, int C, int Hid);
#define DVQ_GATE_LDS_MAX (160 * 1024 - 256)   // dynamic LDS the direct form of the gate opts in to (its static LDS takes the rest)
size_t dvq_router_gate_lds_bytes(int nb, int C, int hc, int wc, int groups, int Hid, int act);
int dvq_launch_router_gate_prepare(const float *W1, int nb, int C, int Hid, void *prep, hipStream_t st);
int dvq_launch_restart_pick(unsigned long long seed, long long n, int k, long long *out, hipStream_t st);
int dvq_launch_ema_update(const float *stats_sum, const float *stats_count, float decay, float eps, int K, int D,
                          const float *cs_old, float *cs_new, float *embed_ema, float *weight, int restart, const float *restart_rows,
                          const float *z, int HW, const long long *pick, hipStream_t st);
int dvq_launch_router_gate_prepare_norm(const float *const *gn_w, const float *const *gn_b, int nb, int C, int Hid, void *prep,
                                        hipStream_t st);
// xt: the type of the branch features h (0 = float32, DVQ_DTYPE_F16 / DVQ_DTYPE_BF16: widened where the pooling pass loads them)
// nhwc: the branches are channels_last, [B, rows, cols, C] (DVQ_NHWC: the pooling pass reads them in place)
int dvq_launch_router_gate(int nb, const void *const *h, int xt, int nhwc, const float *const *gn_w, const float *const *gn_b,
                           int B, int C, int hc, int wc, int groups, float eps,
                           const float *W1, const float *b1, const float *W2, const float *b2,
                           int Hid, int act, const void *w1_prep, float *gate, void *ws, hipStream_t st);
size_t dvq_route_train_ws_bytes(int nb, int B, int C, int hc, int wc, int groups, int H);
int dvq_launch_route_train_fwd(const DvqRouteTrain *p, hipStream_t st);
int dvq_launch_route_train_bwd(const DvqRouteTrain *p, hipStream_t st);

int dvq_rq_blocks(long N, int D);
void dvq_rq_layout(long N, int D, int depth, int want_grad, size_t *off_res0, size_t *off_res1, size_t *off_agg, size_t *off_s,
                   size_t *total);
int dvq_launch_rq_step(const float *x, const float *r_in, const float *E, int K, const long long *code, int B, int h, int w,
                       int rH, int rW, int Dl, int i, int depth, int want_grad, long long *codes, float *out, void *ws,
                       hipStream_t st);
int dvq_launch_rq_loss(long N, int D, int depth, const void *ws, float *loss, hipStream_t st);
int dvq_launch_rq_backward(const float *g_out, const float *g_loss, int B, int h, int w, int rH, int rW, int Dl, int depth,
                           const void *ws, float *g_x, hipStream_t st);
int dvq_launch_rq_embed(const float *const *E, const int *K, int depth, const long long *codes, int B, int h, int w, int rH, int rW,
                        int Dl, int mode, int j, float *out, hipStream_t st);
int dvq_launch_soft_assign(const float *x, const float *prep, int D, int K, long N, float temp, const float *q, float *soft,
                           float *dist, float *sbuf, long long *codes, hipStream_t st);
int dvq_launch_score_assign(const float *z, const float *prep, int D, int HW, int K, long N, int metric, float temp, const float *u,
                            long long *codes, hipStream_t st);
int dvq_launch_cdist_sample_assign(const float *z, const float *prep, int D, int HW, int K, long N, float temp, const float *u,
                                   long long *codes, hipStream_t st);
void dvq_ortho_grid(int h, int n, unsigned *gx, unsigned *gy);
int dvq_launch_ortho_forward(const float *t, int h, int n, int D, float *rinv, float *loss, double *partials, hipStream_t st);
void dvq_ortho_backward_slices(int h, int n, int *S, int *tper);
int dvq_launch_ortho_backward(const float *t, const float *rinv, const float *gout, int h, int n, int D, float *grad, float *gpart,
                              hipStream_t st);
int dvq_launch_lucid_update(int kind, const float *counts, const float *sums, float decay, float eps, float threshold, int K, int D,
                            const float *cs_old, float *cs_new, const float *embed_avg, float *embed, const float *x, int HW,
                            long long N, const long long *pick, hipStream_t st);
int dvq_apply_codes_blocks(long N);
int dvq_launch_apply_codes(const float *z, const float *E, const long long *codes, const float *mask, int D, int HW, int K, long N,
                           float *zq, double *partials, hipStream_t st);
int dvq_launch_gumbel_bias(const float *bias, int K, int D, void *prep, hipStream_t st);
int dvq_gumbel_blocks(long N);
int dvq_launch_gumbel_assign(const float *z, const float *prep, const float *E, int C, int HW, int K, int d, long N, float tau,
                             double log_kl_K, const float *q, float *zq, long long *codes, double *partials, hipStream_t st,
                             float *logits = nullptr);    // logits [B, K, HW] given: the training forward, which writes them too
// GumbelQuantize's backward (vq_gumbel_backward.hip; include/dvq.h: dvq_vq_gumbel_backward_f32): dlogits [B, K, HW] from the saved
// logits, the variates q (nullable), u = embed . G (nullable) and the device scalar g_kl (nullable); dlogits may be u itself
int dvq_launch_gumbel_backward(const float *logits, const float *q, const float *u, const float *g_kl, int HW, int K, long N,
                               float tau, float *dlogits, hipStream_t st);
int dvq_narrow_tile_codes(int D);
int dvq_narrow_blocks(long N);
int dvq_launch_narrow(const float *z, const float *E, const float *mask, int D, int HW, int K, long N, bool flat, float *zq,
                      long long *codes, double *partials, hipStream_t st);
int dvq_launch_gumbel_kl_finalize(const double *partials, int nparts, double inv_n, float *kl, hipStream_t st);
size_t dvq_qconv_prep_bytes_impl(int D);
int dvq_launch_qconv_prep(const float *Wt, const float *bias, int D, void *prep, hipStream_t st);
int dvq_launch_qconv(const float *x, const DvqRouted *rv, const void *prep, int D, int HW, long N, float *hout,
                     hipStream_t st);
int dvq_launch_filter_scores_debug(const float *tokens, int n, const void *prep, int D, int K, float *G,
                                   float *thr2W, float *xn, float *scale_b_out, hipStream_t st, int fold = 0);
size_t dvq_xch_bytes(long cpi, long gpi, int b_max, int num_codes);
int dvq_launch_xch_pack(const long long *codes, const long long *grain, const float *loss, double numel, int b_local,
                        int b_max, long cpi, long gpi, int num_codes, void *buf, hipStream_t st);
int dvq_launch_xch_unpack(const void *gathered, int world, int global_batch, long cpi, long gpi, int num_codes,
                          long long *codes, long long *grain, float *mean, hipStream_t st);
