// dvq_abi.hip -- the extern "C" boundary of libdvq.so (see include/dvq.h).
// Argument validation + launch only: no allocation, no synchronisation, no torch types.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

#include "../../include/dvq.h"
#include "launchers.h"

#define DVQ_VERSION 2000   // 0.20.0 (include/dvq.h lists what each version changed)
#define DVQ_ROUTE_MAX_CELLS_ABI 1024   // = DVQ_ROUTE_MAX_CELLS (dvq_filter.h)

static thread_local char g_err[512] = "";

void dvq_set_error(const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

static int hip_rc(int rc, const char *what)
{
    if (rc == 0) return DVQ_OK;
    dvq_set_error("%s: HIP error %d (%s)", what, rc, hipGetErrorString((hipError_t)rc));
    return DVQ_EHIP;
}

static bool dim_ok(int D) { return D == 64 || D == 128 || D == 256; }

// ---- checks whose words repeat from entry point to entry point: each sets the message and returns its status, DVQ_OK to go on.
// A site whose text or status differs in anything (dvq.h promises them as they are) stays written out where it is.
static int null_pointer(const char *fn) { dvq_set_error("%s: null pointer", fn); return DVQ_EINVAL; }

static int check_positive(const char *fn, int B, int HW, int K)
{
    if (B > 0 && HW > 0 && K > 0) return DVQ_OK;
    dvq_set_error("%s: B=%d HW=%d K=%d must be positive", fn, B, HW, K);
    return DVQ_EINVAL;
}

static int check_width(const char *fn, int D)
{
    if (dim_ok(D)) return DVQ_OK;
    dvq_set_error("%s: D=%d unsupported (kernel widths 64, 128, 256; a multiple of 32 below 256 runs EXACTLY at the next width with zero channels appended to latents and codebook, as the Python drop-in does)", fn, D);
    return DVQ_EUNSUPPORTED;
}

// N tokens (below 2^31 where n31) of w0, w1, w2 elements each: every product below 2^40
static int check_size(const char *fn, size_t N, bool n31, size_t w0 = 0, size_t w1 = 0, size_t w2 = 0)
{
    const size_t lim = (size_t)1 << 40;
    if (!(n31 && N >= ((size_t)1 << 31)) && N * w0 < lim && N * w1 < lim && N * w2 < lim) return DVQ_OK;
    dvq_set_error("%s: tensor too large", fn);
    return DVQ_EUNSUPPORTED;
}

static int check_ws_aligned(const char *fn, const void *ws)     // (null passes)
{
    if (((uintptr_t)ws & 255) == 0) return DVQ_OK;
    dvq_set_error("%s: workspace must be 256-byte aligned", fn);
    return DVQ_EINVAL;
}

// a workspace of `need` bytes, then its alignment; null_as_0: a null workspace is reported as 0 bytes
static int check_workspace(const char *fn, const void *ws, size_t ws_bytes, size_t need, bool null_as_0 = false)
{
    if (ws && ws_bytes >= need) return check_ws_aligned(fn, ws);
    dvq_set_error("%s: workspace %zu < %zu bytes", fn, (ws || !null_as_0) ? ws_bytes : (size_t)0, need);
    return DVQ_EWORKSPACE;
}

static int check_prep_buffer(const char *fn, const void *prep, size_t prep_bytes, size_t need)
{
    if (prep_bytes < need) { dvq_set_error("%s: prep buffer %zu < %zu bytes", fn, prep_bytes, need); return DVQ_EWORKSPACE; }
    if (((uintptr_t)prep & 255) != 0) { dvq_set_error("%s: prep must be 256-byte aligned", fn); return DVQ_EINVAL; }
    return DVQ_OK;
}

// the *_x16 entry points: dtype names one of the two 16-bit types
static int check_x16_dtype(const char *fn, int dtype)
{
    if (dtype == DVQ_DTYPE_F16 || dtype == DVQ_DTYPE_BF16) return DVQ_OK;
    dvq_set_error("%s: dtype %d (DVQ_DTYPE_F16 = 1, DVQ_DTYPE_BF16 = 2)", fn, dtype);
    return DVQ_EINVAL;
}

// loss partials: pass 1 / exact blocks (<= 2 ceil(N/128)), resolver blocks (<= max(32, ceil(N/128)))
static size_t partials_bytes_for(long N)
{
    size_t count = 6 * (size_t)((N + 127) / 128) + 160;    // resolver: one per 32 queued-token slots
    return (count * sizeof(double) + 255) / 256 * 256;
}

extern "C" {

int dvq_version(void) { return DVQ_VERSION; }
const char *dvq_last_error_string(void) { return g_err; }

size_t dvq_codebook_prep_bytes(int K, int D)
{
    if (K <= 0 || D <= 0) return 0;
    // f32 tile images + norms + f16 section (images of the filter kernel: 2 B per element + 16 B
    // of per-code metadata), rounded up generously so the layout can grow without an ABI change
    size_t f32 = dvq_prep_f16_offset(K, D);
    size_t f16 = 2 * ((size_t)dvq_num_tiles(K) * 32 * ((size_t)D * 2 + 16) + 4096);   // two tile images (32x32x16 / 16x16x32 order)
    return ((f32 + f16 + 255) / 256) * 256;
}

int dvq_codebook_prepare_f32(const float *codebook, int K, int D, void *prep, size_t prep_bytes,
                             void *stream)
{
    if (!codebook || !prep || K <= 0) { dvq_set_error("dvq_codebook_prepare_f32: null pointer or K <= 0"); return DVQ_EINVAL; }
    if (int rc = check_width("dvq_codebook_prepare_f32", D)) return rc;
    if (int rc = check_prep_buffer("dvq_codebook_prepare_f32", prep, prep_bytes, dvq_codebook_prep_bytes(K, D))) return rc;
    hipStream_t st = (hipStream_t)stream;
    int rc = dvq_launch_prep_f32(codebook, K, D, prep, st);
    if (rc) return hip_rc(rc, "codebook_prep_f32");
    rc = dvq_launch_prep_f16(codebook, K, D, prep, st);
    return hip_rc(rc, "codebook_prep_f16");
}

size_t dvq_vq_assign_workspace_bytes(int B, int D, int HW, int K, int mode)
{
    if (B <= 0 || HW <= 0 || K <= 0 || D <= 0) return 0;
    mode &= ~DVQ_MODE_WS_CLEAN;
    long N = (long)B * HW;
    size_t partials = partials_bytes_for(N);
    size_t extra = (mode == DVQ_MODE_FILTER || mode == DVQ_MODE_FILTER_PASS1 || mode == DVQ_MODE_FILTER_WIDE) ? dvq_filter_ws_extra_bytes(D, HW, K, N) : 0;
    return partials + extra + 256;
}

size_t dvq_vq_assign_fallback_count_offset(int B, int D, int HW, int K)
{
    (void)D; (void)K;
    if (B <= 0 || HW <= 0) return 0;
    long N = (long)B * HW;
    return partials_bytes_for(N);
}

// The dense assign, float32 latents (dtype 0) or 16-bit ones (DVQ_DTYPE_F16 / DVQ_DTYPE_BF16: z read and zq written as that type by
// the same chain of kernels)
static int assign_nchw(const char *fn, int dtype, const void *z, const float *codebook, const void *prep, const float *mask,
                       int B, int D, int HW, int K, float beta, void *zq, int64_t *codes, float *loss,
                       void *ws, size_t ws_bytes, int mode, void *stream)
{
    const bool x16 = dtype != 0;
    if (!z || !codebook || !prep || !codes) return null_pointer(fn);
    if (x16 && (((uintptr_t)z | (uintptr_t)zq) & 1) != 0) { dvq_set_error("%s: z and zq must be 2-byte aligned", fn); return DVQ_EINVAL; }
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    if (x16 && !dim_ok(D)) { dvq_set_error("%s: D=%d unsupported (kernel widths 64, 128, 256; the narrow widths 3, 4, 8, 16 take float32 latents only: dvq_vq_assign_narrow_*_f32)", fn, D); return DVQ_EUNSUPPORTED; }
    if (int rc = check_width(fn, D)) return rc;
    const bool ws_clean = (mode & DVQ_MODE_WS_CLEAN) != 0;
    mode &= ~DVQ_MODE_WS_CLEAN;
    const bool pass1_only = (mode == DVQ_MODE_FILTER_PASS1);
    const bool force_wide = (mode == DVQ_MODE_FILTER_WIDE);
    if (x16 && (pass1_only || force_wide)) { dvq_set_error("%s: mode %d (pass 1 alone / the wide form) exists for float32 latents only", fn, mode); return DVQ_EUNSUPPORTED; }
    if (pass1_only || force_wide) mode = DVQ_MODE_FILTER;
    if (mode != DVQ_MODE_EXACT && mode != DVQ_MODE_FILTER) { dvq_set_error("%s: unknown mode %d", fn, mode); return DVQ_EINVAL; }
    if (int rc = check_size(fn, (size_t)B * HW, false, D)) return rc;
    const long N = (long)B * HW;
    if (loss && !ws) { dvq_set_error("%s: loss requested without workspace", fn); return DVQ_EINVAL; }
    if (int rc = (loss || mode == DVQ_MODE_FILTER) ? check_workspace(fn, ws, ws_bytes, dvq_vq_assign_workspace_bytes(B, D, HW, K, mode))
                                                   : check_ws_aligned(fn, ws)) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *partials = loss ? (double *)ws : nullptr;
    if (mode == DVQ_MODE_FILTER && dvq_filter_supported(D, HW, K, N)) {
        const int rc = dvq_launch_filter((const float *)z, prep, codebook, mask, D, HW, K, N, (float *)zq, (long long *)codes, partials,
                                         (char *)ws + partials_bytes_for(N), pass1_only, force_wide, loss, beta, nullptr, st, nullptr,
                                         nullptr, ws_clean, dtype);
        return hip_rc(rc, x16 ? "vq_assign_filter_x16" : "vq_assign_filter");     // the loss finalize is fused into its last kernel
    }
    int rc = dvq_launch_exact((const float *)z, (const float *)prep, codebook, mask, D, HW, K, N, (float *)zq, (long long *)codes, partials,
                              nullptr, st, dtype);
    if (rc) return hip_rc(rc, x16 ? "vq_assign_exact_x16" : "vq_assign_exact");
    if (loss) {
        rc = dvq_launch_loss_finalize(partials, (int)((N + 127) / 128), 1.0 / ((double)N * D), beta, loss, st);
        if (rc) return hip_rc(rc, "vq_loss_finalize");
    }
    return DVQ_OK;
}

int dvq_vq_assign_nchw_f32(const float *z, const float *codebook, const void *prep,
                           const float *mask, int B, int D, int HW, int K, float beta,
                           float *zq, int64_t *codes, float *loss,
                           void *ws, size_t ws_bytes, int mode, void *stream)
{
    return assign_nchw("dvq_vq_assign_nchw_f32", 0, z, codebook, prep, mask, B, D, HW, K, beta, zq, codes, loss, ws, ws_bytes, mode, stream);
}

int dvq_vq_assign_nchw_x16(const void *z, int dtype, const float *codebook, const void *prep, const float *mask,
                           int B, int D, int HW, int K, float beta, void *zq, int64_t *codes, float *loss,
                           void *ws, size_t ws_bytes, int mode, void *stream)
{
    const char *fn = "dvq_vq_assign_nchw_x16";
    if (int rc = check_x16_dtype(fn, dtype)) return rc;
    return assign_nchw(fn, dtype, z, codebook, prep, mask, B, D, HW, K, beta, zq, codes, loss, ws, ws_bytes, mode, stream);
}

// row-major latents: the same op on [N, D, 1] (the filter path reads / writes a token's row with 16-byte accesses when HW == 1)
int dvq_vq_assign_flat_f32(const float *z, const float *codebook, const void *prep, const float *mask,
                           int64_t N, int D, int K, float beta, float *zq, int64_t *codes, float *loss,
                           void *ws, size_t ws_bytes, int mode, void *stream)
{
    if (N <= 0 || N >= ((int64_t)1 << 31)) { dvq_set_error("dvq_vq_assign_flat_f32: N=%lld out of range", (long long)N); return DVQ_EINVAL; }
    return dvq_vq_assign_nchw_f32(z, codebook, prep, mask, (int)N, D, 1, K, beta, zq, codes, loss, ws, ws_bytes, mode, stream);
}

// ---- the 1x1 quant_conv fused into the assign (filter mode; D = 256) --------------------------------------------------
static int conv_desc(const char *fn, const void *qconv_prep, float *h_buf, int h_all, int D, DvqConv *cv)
{
    if (!qconv_prep) { dvq_set_error("%s: qconv_prep is required", fn); return DVQ_EINVAL; }
    if (h_all && !h_buf) { dvq_set_error("%s: h_all needs an h_buf", fn); return DVQ_EINVAL; }
    if (D != 256) { dvq_set_error("%s: the fused conv exists for D = 256 (got %d): use dvq_qconv_f32 + dvq_vq_assign_nchw_f32", fn, D); return DVQ_EUNSUPPORTED; }
    if (((uintptr_t)qconv_prep & 255) != 0 || ((uintptr_t)h_buf & 3) != 0) { dvq_set_error("%s: qconv_prep must be 256-byte aligned", fn); return DVQ_EINVAL; }
    cv->meta = (const QconvMeta *)qconv_prep;
    cv->wimg = (const char *)qconv_prep + 256;
    cv->bias = (const float *)((const char *)qconv_prep + 256 + (size_t)(D / 32) * qconv_tile_bytes(D));
    cv->h_buf = h_all ? h_buf : nullptr;                     // (without h_all the op touches no h_buf: nullable since 0.6.0)
    cv->h_all = h_all ? 1 : 0;
    return DVQ_OK;
}

int dvq_vq_assign_qconv_f32(const float *x, const void *qconv_prep, const float *codebook, const void *prep,
                            const float *mask, int B, int D, int HW, int K, float beta,
                            float *zq, int64_t *codes, float *loss, float *h_buf, int h_all,
                            void *ws, size_t ws_bytes, int mode, void *stream)
{
    const char *fn = "dvq_vq_assign_qconv_f32";
    if (!x || !codebook || !prep || !codes) return null_pointer(fn);
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    const bool ws_clean = (mode & DVQ_MODE_WS_CLEAN) != 0;
    mode &= ~DVQ_MODE_WS_CLEAN;
    const bool pass1_only = (mode == DVQ_MODE_FILTER_PASS1);
    if (mode != DVQ_MODE_FILTER && !pass1_only) { dvq_set_error("%s: mode %d (the conv is fused into the filter path only)", fn, mode); return DVQ_EINVAL; }
    DvqConv cv;
    int rc = conv_desc(fn, qconv_prep, h_buf, h_all, D, &cv);
    if (rc) return rc;
    const long N = (long)B * HW;
    if (int rc = check_size(fn, (size_t)N, true, D)) return rc;
    if (!dvq_filter_supported(D, HW, K, N)) { dvq_set_error("%s: shape unsupported by the filter path (D=%d HW=%d K=%d: K < 2^20, D * HW < 2^29)", fn, D, HW, K); return DVQ_EUNSUPPORTED; }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_vq_assign_workspace_bytes(B, D, HW, K, DVQ_MODE_FILTER))) return rc;
    double *partials = loss ? (double *)ws : nullptr;
    rc = dvq_launch_filter(x, prep, codebook, mask, D, HW, K, N, zq, (long long *)codes, partials,
                           (char *)ws + partials_bytes_for(N), pass1_only, false, loss, beta, nullptr, (hipStream_t)stream, &cv, nullptr, ws_clean);
    return hip_rc(rc, fn);
}

// ---- the conv folded into the codebook (vq_fold.hip; filter path, codes [+ z_q := e[code]], no loss) -------------------------
static int fold_desc(const char *fn, const void *qconv_prep, const void *fold_prep, int D, DvqFold *fd)
{
    if (!qconv_prep || !fold_prep) { dvq_set_error("%s: qconv_prep and fold_prep are required", fn); return DVQ_EINVAL; }
    if (((uintptr_t)qconv_prep & 255) != 0 || ((uintptr_t)fold_prep & 255) != 0) { dvq_set_error("%s: qconv_prep / fold_prep must be 256-byte aligned", fn); return DVQ_EINVAL; }
    fd->fprep = (const char *)fold_prep;
    fd->cv.meta = (const QconvMeta *)qconv_prep;
    fd->cv.wimg = (const char *)qconv_prep + 256;
    fd->cv.bias = (const float *)((const char *)qconv_prep + 256 + (size_t)(D / 32) * qconv_tile_bytes(D));
    fd->cv.h_buf = nullptr;
    fd->cv.h_all = 0;
    return DVQ_OK;
}

size_t dvq_fold_prep_bytes(int K, int D)
{
    if (K <= 0 || !dim_ok(D)) return 0;
    return (dvq_fold_prep_bytes_impl(K, D) + 255) / 256 * 256;
}

int dvq_fold_prepare_f32(const float *codebook, int K, int D, const void *codebook_prep, const float *conv_weight,
                         const float *conv_bias, void *fold_prep, size_t fold_prep_bytes, void *stream)
{
    const char *fn = "dvq_fold_prepare_f32";
    if (!codebook || !codebook_prep || !conv_weight || !fold_prep || K <= 0) { dvq_set_error("%s: null pointer or K <= 0", fn); return DVQ_EINVAL; }
    if (int rc = check_width(fn, D)) return rc;
    if (fold_prep_bytes < dvq_fold_prep_bytes(K, D)) { dvq_set_error("%s: fold_prep buffer %zu < %zu bytes", fn, fold_prep_bytes, dvq_fold_prep_bytes(K, D)); return DVQ_EWORKSPACE; }
    if (((uintptr_t)fold_prep & 255) != 0 || ((uintptr_t)codebook_prep & 255) != 0) { dvq_set_error("%s: prep buffers must be 256-byte aligned", fn); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_fold_prep(codebook, K, D, codebook_prep, conv_weight, conv_bias, fold_prep, (hipStream_t)stream), fn);
}

int dvq_vq_assign_fold_f32(const float *x, const void *qconv_prep, const void *fold_prep, const float *codebook,
                           const void *prep, int B, int D, int HW, int K, float *zq, int64_t *codes,
                           void *ws, size_t ws_bytes, int mode, void *stream)
{
    const char *fn = "dvq_vq_assign_fold_f32";
    const bool ws_clean = (mode & DVQ_MODE_WS_CLEAN) != 0;
    mode &= ~DVQ_MODE_WS_CLEAN;
    if (!x || !codebook || !prep || !codes) return null_pointer(fn);
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    if (int rc = check_width(fn, D)) return rc;
    DvqFold fd;
    int rc = fold_desc(fn, qconv_prep, fold_prep, D, &fd);
    if (rc) return rc;
    const long N = (long)B * HW;
    if (int rc = check_size(fn, (size_t)N, true, D)) return rc;
    if (!dvq_filter_supported(D, HW, K, N)) { dvq_set_error("%s: shape unsupported by the filter path (D=%d HW=%d K=%d: K < 2^20, D * HW < 2^29)", fn, D, HW, K); return DVQ_EUNSUPPORTED; }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_vq_assign_workspace_bytes(B, D, HW, K, DVQ_MODE_FILTER))) return rc;
    if (mode != DVQ_MODE_FILTER && mode != DVQ_MODE_FILTER_PASS1) { dvq_set_error("%s: mode %d (the fold is a form of the filter path)", fn, mode); return DVQ_EINVAL; }
    rc = dvq_launch_filter(x, prep, codebook, nullptr, D, HW, K, N, zq, (long long *)codes, nullptr,
                           (char *)ws + partials_bytes_for(N), mode == DVQ_MODE_FILTER_PASS1, false, nullptr, 0.0f, nullptr,
                           (hipStream_t)stream, nullptr, &fd, ws_clean);
    return hip_rc(rc, fn);
}

// token ids of a routed batch: at most one per output position
static long routed_ids(int nb, int B, long N) { (void)nb; (void)B; return N; }

static int routed_dims(int nb, int hc, int wc, int *SC)
{
    *SC = (nb == 2) ? 2 : 4;
    return (nb == 2 || nb == 3) && hc > 0 && wc > 0 && (long)hc * wc <= DVQ_ROUTE_MAX_CELLS_ABI;
}

size_t dvq_vq_assign_routed_workspace_bytes(int num_branches, int B, int D, int hc, int wc, int K, int mode)
{
    int SC;
    if (B <= 0 || D <= 0 || K <= 0 || !routed_dims(num_branches, hc, wc, &SC)) return 0;
    const int HWout = SC * hc * SC * wc;
    const long N = (long)B * HWout;
    (void)mode;                                          // sized for the filter path in every mode
    return partials_bytes_for(routed_ids(num_branches, B, N)) + dvq_filter_ws_extra_bytes(D, HWout, K, N) + 256;
}

size_t dvq_vq_assign_routed_fallback_count_offset(int num_branches, int B, int D, int hc, int wc, int K)
{
    int SC;
    (void)D; (void)K;
    if (B <= 0 || !routed_dims(num_branches, hc, wc, &SC)) return 0;
    return partials_bytes_for(routed_ids(num_branches, B, (long)B * SC * hc * SC * wc));
}

static int routed_common(const char *fn, int nb, const void *gate, int gate_kind, float threshold,
                         const float *h_coarse, const float *h_median, const float *h_fine,
                         const float *codebook, const void *prep, int B, int D, int hc, int wc, int K, float beta,
                         float *zq, int64_t *codes, float *loss, int64_t *indices, float *cmask, int64_t *gate_out,
                         void *ws, size_t ws_bytes, int mode, void *stream,
                         const void *qconv_prep = nullptr, float *h_buf = nullptr, int h_all = 0, bool conv = false,
                         const void *fold_prep = nullptr)
{
    if (!gate || !h_coarse || !h_fine || !codebook || !prep || !codes || !indices || !cmask || (nb == 3 && !h_median)) {
        return null_pointer(fn);
    }
    if (B <= 0 || hc <= 0 || wc <= 0 || K <= 0) { dvq_set_error("%s: B=%d hc=%d wc=%d K=%d must be positive", fn, B, hc, wc, K); return DVQ_EINVAL; }
    if (gate_kind != DVQ_GATE_F32 && gate_kind != DVQ_GATE_I64 && gate_kind != DVQ_GATE_ENTROPY) { dvq_set_error("%s: gate_kind %d", fn, gate_kind); return DVQ_EINVAL; }
    if (gate_kind == DVQ_GATE_ENTROPY && nb != 2) { dvq_set_error("%s: the entropy gate is a dual-granularity router", fn); return DVQ_EINVAL; }
    if (int rc = check_width(fn, D)) return rc;
    int SC;
    if (!routed_dims(nb, hc, wc, &SC)) { dvq_set_error("%s: hc*wc=%ld exceeds %d coarse cells", fn, (long)hc * wc, DVQ_ROUTE_MAX_CELLS_ABI); return DVQ_EUNSUPPORTED; }
    const bool ws_clean = (mode & DVQ_MODE_WS_CLEAN) != 0;
    mode &= ~DVQ_MODE_WS_CLEAN;
    const bool pass1_only = (mode == DVQ_MODE_FILTER_PASS1);
    if (pass1_only) mode = DVQ_MODE_FILTER;
    if (mode != DVQ_MODE_EXACT && mode != DVQ_MODE_FILTER) { dvq_set_error("%s: unknown mode %d", fn, mode); return DVQ_EINVAL; }
    DvqConv cv;
    if (conv) {
        if (mode != DVQ_MODE_FILTER) { dvq_set_error("%s: mode %d (the conv is fused into the filter path only)", fn, mode); return DVQ_EINVAL; }
        const int rcv = conv_desc(fn, qconv_prep, h_buf, h_all, D, &cv);
        if (rcv) return rcv;
    }
    DvqFold fd;
    if (fold_prep != nullptr) {
        if (mode != DVQ_MODE_FILTER) { dvq_set_error("%s: mode %d (the fold is a form of the filter path)", fn, mode); return DVQ_EINVAL; }
        const int rcf = fold_desc(fn, qconv_prep, fold_prep, D, &fd);
        if (rcf) return rcf;
    }
    const long N = (long)B * SC * hc * SC * wc;
    if (N >= (1L << 31) || (size_t)N * D >= ((size_t)1 << 40) || B > 32768) { dvq_set_error("%s: tensor too large", fn); return DVQ_EUNSUPPORTED; }
    if (!dvq_filter_supported(D, SC * hc * SC * wc, K, N)) { dvq_set_error("%s: shape unsupported by the filter path (D=%d HW=%d K=%d: K < 2^20, D * HW < 2^29)", fn, D, SC * hc * SC * wc, K); return DVQ_EUNSUPPORTED; }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_vq_assign_routed_workspace_bytes(nb, B, D, hc, wc, K, mode))) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *partials = loss ? (double *)ws : nullptr;
    const size_t pbytes = partials_bytes_for(routed_ids(nb, B, N));
    const int gmode = (gate_kind == DVQ_GATE_ENTROPY) ? 2 : (gate_kind == DVQ_GATE_I64 ? 1 : 0);
    int rc = dvq_launch_routed(nb, gmode, gate, threshold, h_coarse, h_median, h_fine, prep, codebook, B, D, hc, wc, K,
                               beta, zq, (long long *)codes, loss, (long long *)indices, cmask, (long long *)gate_out,
                               partials, (char *)ws + pbytes, mode == DVQ_MODE_EXACT, pass1_only, st, conv ? &cv : nullptr,
                               fold_prep != nullptr ? &fd : nullptr, ws_clean);
    return hip_rc(rc, fn);                                   // the loss finalize is part of the op in both modes
}

int dvq_vq_assign_routed_dual_f32(const void *gate, int gate_kind, float threshold,
                                  const float *h_coarse, const float *h_fine,
                                  const float *codebook, const void *prep,
                                  int B, int D, int hc, int wc, int K, float beta,
                                  float *zq, int64_t *codes, float *loss,
                                  int64_t *indices, float *cmask, int64_t *gate_out,
                                  void *ws, size_t ws_bytes, int mode, void *stream)
{
    return routed_common("dvq_vq_assign_routed_dual_f32", 2, gate, gate_kind, threshold, h_coarse, nullptr, h_fine,
                         codebook, prep, B, D, hc, wc, K, beta, zq, codes, loss, indices, cmask, gate_out, ws, ws_bytes,
                         mode, stream);
}

int dvq_vq_assign_routed_triple_f32(const void *gate, int gate_kind,
                                    const float *h_coarse, const float *h_median, const float *h_fine,
                                    const float *codebook, const void *prep,
                                    int B, int D, int hc, int wc, int K, float beta,
                                    float *zq, int64_t *codes, float *loss,
                                    int64_t *indices, float *cmask,
                                    void *ws, size_t ws_bytes, int mode, void *stream)
{
    if (!h_median) { dvq_set_error("dvq_vq_assign_routed_triple_f32: null h_median"); return DVQ_EINVAL; }
    return routed_common("dvq_vq_assign_routed_triple_f32", 3, gate, gate_kind, 0.0f, h_coarse, h_median, h_fine,
                         codebook, prep, B, D, hc, wc, K, beta, zq, codes, loss, indices, cmask, nullptr, ws, ws_bytes,
                         mode, stream);
}

int dvq_vq_assign_routed_qconv_dual_f32(const void *gate, int gate_kind, float threshold,
                                        const float *h_coarse, const float *h_fine, const void *qconv_prep,
                                        const float *codebook, const void *prep,
                                        int B, int D, int hc, int wc, int K, float beta,
                                        float *zq, int64_t *codes, float *loss,
                                        int64_t *indices, float *cmask, int64_t *gate_out, float *h_buf, int h_all,
                                        void *ws, size_t ws_bytes, int mode, void *stream)
{
    return routed_common("dvq_vq_assign_routed_qconv_dual_f32", 2, gate, gate_kind, threshold, h_coarse, nullptr, h_fine,
                         codebook, prep, B, D, hc, wc, K, beta, zq, codes, loss, indices, cmask, gate_out, ws, ws_bytes,
                         mode, stream, qconv_prep, h_buf, h_all, true);
}

int dvq_vq_assign_routed_qconv_triple_f32(const void *gate, int gate_kind,
                                          const float *h_coarse, const float *h_median, const float *h_fine,
                                          const void *qconv_prep, const float *codebook, const void *prep,
                                          int B, int D, int hc, int wc, int K, float beta,
                                          float *zq, int64_t *codes, float *loss,
                                          int64_t *indices, float *cmask, float *h_buf, int h_all,
                                          void *ws, size_t ws_bytes, int mode, void *stream)
{
    if (!h_median) { dvq_set_error("dvq_vq_assign_routed_qconv_triple_f32: null h_median"); return DVQ_EINVAL; }
    return routed_common("dvq_vq_assign_routed_qconv_triple_f32", 3, gate, gate_kind, 0.0f, h_coarse, h_median, h_fine,
                         codebook, prep, B, D, hc, wc, K, beta, zq, codes, loss, indices, cmask, nullptr, ws, ws_bytes,
                         mode, stream, qconv_prep, h_buf, h_all, true);
}

int dvq_vq_assign_routed_fold_dual_f32(const void *gate, int gate_kind, float threshold,
                                       const float *h_coarse, const float *h_fine, const void *qconv_prep,
                                       const void *fold_prep, const float *codebook, const void *prep,
                                       int B, int D, int hc, int wc, int K, float *zq, int64_t *codes,
                                       int64_t *indices, float *cmask, int64_t *gate_out,
                                       void *ws, size_t ws_bytes, int mode, void *stream)
{
    const char *fn = "dvq_vq_assign_routed_fold_dual_f32";
    if (!fold_prep) { dvq_set_error("%s: null fold_prep", fn); return DVQ_EINVAL; }
    return routed_common(fn, 2, gate, gate_kind, threshold, h_coarse, nullptr, h_fine, codebook, prep, B, D, hc, wc, K, 0.0f,
                         zq, codes, nullptr, indices, cmask, gate_out, ws, ws_bytes, mode, stream, qconv_prep,
                         nullptr, 0, false, fold_prep);
}

int dvq_vq_assign_routed_fold_triple_f32(const void *gate, int gate_kind,
                                         const float *h_coarse, const float *h_median, const float *h_fine,
                                         const void *qconv_prep, const void *fold_prep, const float *codebook, const void *prep,
                                         int B, int D, int hc, int wc, int K, float *zq, int64_t *codes,
                                         int64_t *indices, float *cmask, void *ws, size_t ws_bytes, int mode, void *stream)
{
    const char *fn = "dvq_vq_assign_routed_fold_triple_f32";
    if (!h_median || !fold_prep) { dvq_set_error("%s: null h_median / fold_prep", fn); return DVQ_EINVAL; }
    return routed_common(fn, 3, gate, gate_kind, 0.0f, h_coarse, h_median, h_fine, codebook, prep, B, D, hc, wc, K, 0.0f,
                         zq, codes, nullptr, indices, cmask, nullptr, ws, ws_bytes, mode, stream, qconv_prep,
                         nullptr, 0, false, fold_prep);
}

// dtype 0: float32 z, g_zq and g_z; DVQ_DTYPE_F16 / DVQ_DTYPE_BF16: all three of that type
static int backward_nchw(const char *fn, int dtype, const void *z, const float *codebook, const int64_t *codes, const float *mask,
                         const void *g_zq, const float *g_loss, float coef_scale, int B, int D, int HW, int K, void *g_z, void *stream)
{
    if (!z || !codebook || !codes || !g_z) return null_pointer(fn);
    if (!g_zq && !g_loss) { dvq_set_error("%s: neither g_zq nor g_loss given", fn); return DVQ_EINVAL; }
    if (B <= 0 || HW <= 0 || K <= 0 || D <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (D % 16 != 0) { dvq_set_error("%s: D=%d must be a multiple of 16", fn, D); return DVQ_EUNSUPPORTED; }
    if ((((uintptr_t)codebook) & 15) != 0) { dvq_set_error("%s: codebook must be 16-byte aligned", fn); return DVQ_EINVAL; }
    if (dtype != 0 && (((uintptr_t)z | (uintptr_t)g_zq | (uintptr_t)g_z) & 1) != 0) { dvq_set_error("%s: z, g_zq and g_z must be 2-byte aligned", fn); return DVQ_EINVAL; }
    // HW == 1 is a row-major matrix [B, D]: the kernel whose lanes own 16-byte pieces of a row (train_rows.hip), where its pieces are aligned
    if (HW == 1 && (((uintptr_t)z | (uintptr_t)g_zq | (uintptr_t)g_z) & 15) == 0)
        return hip_rc(dvq_launch_vq_backward_rows(z, dtype, codebook, (const long long *)codes, mask, g_zq, g_loss, coef_scale, D, K, (long)B,
                                                  g_z, (hipStream_t)stream), fn);
    return hip_rc(dvq_launch_vq_backward_z(z, dtype, codebook, (const long long *)codes, mask, g_zq, g_loss, coef_scale, D, HW, K,
                                           (long)B * HW, g_z, (hipStream_t)stream), fn);
}

int dvq_vq_backward_nchw_f32(const float *z, const float *codebook, const int64_t *codes, const float *mask,
                             const float *g_zq, const float *g_loss, float coef_scale,
                             int B, int D, int HW, int K, float *g_z, void *stream)
{
    return backward_nchw("dvq_vq_backward_nchw_f32", 0, z, codebook, codes, mask, g_zq, g_loss, coef_scale, B, D, HW, K, g_z, stream);
}

int dvq_vq_backward_nchw_x16(const void *z, int dtype, const float *codebook, const int64_t *codes, const float *mask,
                             const void *g_zq, const float *g_loss, float coef_scale, int B, int D, int HW, int K,
                             void *g_z, void *stream)
{
    const char *fn = "dvq_vq_backward_nchw_x16";
    if (int rc = check_x16_dtype(fn, dtype)) return rc;
    return backward_nchw(fn, dtype, z, codebook, codes, mask, g_zq, g_loss, coef_scale, B, D, HW, K, g_z, stream);
}

int dvq_vq_backward_codebook_nchw_f32(const float *z, const float *codebook, const int64_t *codes, const float *mask,
                                      const float *g_loss, float coef_scale, int B, int D, int HW, int K,
                                      float *g_weight, void *stream)
{
    const char *fn = "dvq_vq_backward_codebook_nchw_f32";
    if (!z || !codebook || !codes || !g_loss || !g_weight) return null_pointer(fn);
    if (B <= 0 || HW <= 0 || K <= 0 || D <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (K > 8192) { dvq_set_error("%s: K=%d > 8192 (index_add the differences instead)", fn, K); return DVQ_EUNSUPPORTED; }
    if (HW == 1)                                            // row-major [B, D]: lane = channel straight from the rows, no LDS transpose
        return hip_rc(dvq_launch_codebook_grad_rows(z, codebook, (const long long *)codes, mask, g_loss, coef_scale, D, (long)B, K, g_weight,
                                                    (hipStream_t)stream), fn);
    return hip_rc(dvq_launch_codebook_grad(z, codebook, (const long long *)codes, mask, g_loss, coef_scale, D, HW, (long)B * HW, K,
                                           g_weight, (hipStream_t)stream), fn);
}

int dvq_embed_gather_f32(const float *codebook, int K, int D, const int64_t *idx, int64_t n,
                         float *out, void *stream)
{
    if (!codebook || !idx || !out) return null_pointer("dvq_embed_gather_f32");
    if (K <= 0 || D <= 0 || n < 0) { dvq_set_error("dvq_embed_gather_f32: bad sizes"); return DVQ_EINVAL; }
    if (D % 4 != 0) { dvq_set_error("dvq_embed_gather_f32: D=%d must be a multiple of 4", D); return DVQ_EUNSUPPORTED; }
    if (n == 0) return DVQ_OK;
    return hip_rc(dvq_launch_embed_gather(codebook, K, D, (const long long *)idx, (long)n, out, (hipStream_t)stream), "embed_gather");
}

int dvq_entropy_gate_f32(const float *entropy, int64_t n, float thr, int64_t *gate, void *stream)
{
    if (!entropy || !gate) return null_pointer("dvq_entropy_gate_f32");
    if (n < 0) { dvq_set_error("dvq_entropy_gate_f32: n < 0"); return DVQ_EINVAL; }
    if (n == 0) return DVQ_OK;
    return hip_rc(dvq_launch_entropy_gate(entropy, (long)n, thr, (long long *)gate, (hipStream_t)stream), "entropy_gate");
}

// DVQ_FEATURES(dtype) and DVQ_NHWC OR-ed into the one enumerated argument of the select / gate entry points: the enumerator is the
// low byte, the feature dtype bits 8 - 11 (0 = float32), the layout bit 12 (DVQ_NHWC: channels_last branches); nothing above it.
// A negative value carries no flag: it is an unknown enumerator as a whole.
static int enum_of(int v) { return v < 0 ? v : (v & 0xFF); }
static int features_of(int v) { return v < 0 ? 0 : ((v >> 8) & 0xF); }
static int layout_of(int v) { return v < 0 ? 0 : ((v >> 12) & 1); }

static int check_features(const char *fn, int xt)
{
    if (xt == 0 || xt == DVQ_DTYPE_F16 || xt == DVQ_DTYPE_BF16) return DVQ_OK;
    dvq_set_error("%s: DVQ_FEATURES dtype %d (0 = float32, DVQ_DTYPE_F16 = 1, DVQ_DTYPE_BF16 = 2)", fn, xt);
    return DVQ_EINVAL;
}

// the bits of the argument that no flag owns (checked after the enumerator, before the dtype)
static int check_flag_bits(const char *fn, int v)
{
    if (v < 0 || (v >> 13) == 0) return DVQ_OK;
    dvq_set_error("%s: flag bits 0x%x above DVQ_NHWC (the argument carries an enumerator, DVQ_FEATURES(dtype) and DVQ_NHWC)", fn, v & ~0x1FFF);
    return DVQ_EINVAL;
}

// gate_dtype: DVQ_GATE_F32 / DVQ_GATE_I64, with DVQ_FEATURES(dtype) for 2-byte features (a, b, h_out then hold such elements)
static int route_args_ok(const char *fn, const void *gate, int gate_dtype, const void *a, const void *b,
                         int B, int C, int hc, int wc, void *h_out, int64_t *indices, float *cmask)
{
    if (!gate || !a || !b || !h_out || !indices || !cmask) return null_pointer(fn);
    const int gd = enum_of(gate_dtype);
    if (gd != DVQ_GATE_F32 && gd != DVQ_GATE_I64) { dvq_set_error("%s: gate_dtype %d", fn, gd); return DVQ_EINVAL; }
    if (int rc = check_flag_bits(fn, gate_dtype)) return rc;
    if (int rc = check_features(fn, features_of(gate_dtype))) return rc;
    if (B <= 0 || C <= 0 || hc <= 0 || wc <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (features_of(gate_dtype) != 0 && (((uintptr_t)a | (uintptr_t)b | (uintptr_t)h_out) & 1) != 0) {
        dvq_set_error("%s: 16-bit features must be 2-byte aligned", fn); return DVQ_EINVAL;
    }
    // DVQ_NHWC: a workgroup numbers the pieces (2 bytes at least) of one row of output pixels with 32 bits
    if (layout_of(gate_dtype) && (double)wc * 4.0 * (double)C * 4.0 >= 2147483648.0) {
        dvq_set_error("%s: DVQ_NHWC: a row of %d cells x C=%d is too long (16 * wc * C < 2^31)", fn, wc, C); return DVQ_EUNSUPPORTED;
    }
    return DVQ_OK;
}

// bytes per feature element of a flagged argument
static int feature_bytes(int v) { return features_of(v) != 0 ? 2 : 4; }

int dvq_route_select_dual_f32(const void *gate, int gate_dtype, const void *h_coarse,
                              const void *h_fine, int B, int C, int hc, int wc,
                              void *h_out, int64_t *indices, float *cmask, void *stream)
{
    int rc = route_args_ok("dvq_route_select_dual_f32", gate, gate_dtype, h_coarse, h_fine, B, C, hc, wc, h_out, indices, cmask);
    if (rc) return rc;
    const int gate_mode = enum_of(gate_dtype) == DVQ_GATE_I64;
    if (layout_of(gate_dtype))
        return hip_rc(dvq_launch_route_select_rows(2, gate_mode, gate, h_coarse, nullptr, h_fine, feature_bytes(gate_dtype), B, C, hc, wc,
                                                   h_out, (long long *)indices, cmask, (hipStream_t)stream), "route_select_dual");
    if (features_of(gate_dtype) != 0)
        return hip_rc(dvq_launch_route_select_x16(2, gate_mode, gate, h_coarse, nullptr, h_fine, B, C, hc, wc, h_out,
                                                  (long long *)indices, cmask, (hipStream_t)stream), "route_select_dual");
    return hip_rc(dvq_launch_route_select(2, gate_mode, gate, (const float *)h_coarse, nullptr, (const float *)h_fine, B, C, hc, wc,
                                          (float *)h_out, (long long *)indices, cmask, 0.0f, nullptr, (hipStream_t)stream), "route_select_dual");
}

int dvq_route_select_dual_entropy_f32(const float *entropy, float threshold, const float *h_coarse,
                                      const float *h_fine, int B, int C, int hc, int wc,
                                      float *h_out, int64_t *indices, float *cmask, int64_t *gate_out,
                                      void *stream)
{
    int rc = route_args_ok("dvq_route_select_dual_entropy_f32", entropy, DVQ_GATE_F32, h_coarse, h_fine, B, C, hc, wc, h_out, indices, cmask);
    if (rc) return rc;
    return hip_rc(dvq_launch_route_select(2, 2, entropy, h_coarse, nullptr, h_fine, B, C, hc, wc,
                                          h_out, (long long *)indices, cmask, threshold, (long long *)gate_out,
                                          (hipStream_t)stream), "route_select_dual_entropy");
}

int dvq_route_select_triple_f32(const void *gate, int gate_dtype, const void *h_coarse,
                                const void *h_median, const void *h_fine, int B, int C, int hc,
                                int wc, void *h_out, int64_t *indices, float *cmask, void *stream)
{
    int rc = route_args_ok("dvq_route_select_triple_f32", gate, gate_dtype, h_coarse, h_fine, B, C, hc, wc, h_out, indices, cmask);
    if (rc) return rc;
    if (!h_median) { dvq_set_error("dvq_route_select_triple_f32: null h_median"); return DVQ_EINVAL; }
    const int gate_mode = enum_of(gate_dtype) == DVQ_GATE_I64;
    if (features_of(gate_dtype) != 0 && ((uintptr_t)h_median & 1) != 0) {
        dvq_set_error("dvq_route_select_triple_f32: 16-bit features must be 2-byte aligned"); return DVQ_EINVAL;
    }
    if (layout_of(gate_dtype))
        return hip_rc(dvq_launch_route_select_rows(3, gate_mode, gate, h_coarse, h_median, h_fine, feature_bytes(gate_dtype), B, C, hc, wc,
                                                   h_out, (long long *)indices, cmask, (hipStream_t)stream), "route_select_triple");
    if (features_of(gate_dtype) != 0) {
        return hip_rc(dvq_launch_route_select_x16(3, gate_mode, gate, h_coarse, h_median, h_fine, B, C, hc, wc, h_out,
                                                  (long long *)indices, cmask, (hipStream_t)stream), "route_select_triple");
    }
    return hip_rc(dvq_launch_route_select(3, gate_mode, gate, (const float *)h_coarse, (const float *)h_median, (const float *)h_fine,
                                          B, C, hc, wc, (float *)h_out, (long long *)indices, cmask, 0.0f, nullptr, (hipStream_t)stream),
                  "route_select_triple");
}

static int ema_accumulate_nchw(const char *fn, int dtype, const void *z, const int64_t *codes, int B, int D, int HW, int K,
                               float *cluster_size, float *vectors_sum, void *stream)
{
    if (!z || !codes || !cluster_size || !vectors_sum) return null_pointer(fn);
    if (dtype != 0 && ((uintptr_t)z & 1) != 0) { dvq_set_error("%s: z must be 2-byte aligned", fn); return DVQ_EINVAL; }
    if (B <= 0 || D <= 0 || HW <= 0 || K <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (HW == 1)                                            // row-major [B, D] (train_rows.hip; any K)
        return hip_rc(dvq_launch_ema_accumulate_rows(z, dtype, (const long long *)codes, D, (long)B, K, cluster_size, vectors_sum,
                                                     (hipStream_t)stream), dtype != 0 ? fn : "ema_accumulate");
    return hip_rc(dvq_launch_ema_accumulate(z, dtype, (const long long *)codes, D, HW, (long)B * HW, K, cluster_size, vectors_sum,
                                            (hipStream_t)stream), dtype != 0 ? fn : "ema_accumulate");
}

int dvq_ema_accumulate_nchw_f32(const float *z, const int64_t *codes, int B, int D, int HW, int K,
                                float *cluster_size, float *vectors_sum, void *stream)
{
    return ema_accumulate_nchw("dvq_ema_accumulate_nchw_f32", 0, z, codes, B, D, HW, K, cluster_size, vectors_sum, stream);
}

int dvq_ema_accumulate_nchw_x16(const void *z, int dtype, const int64_t *codes, int B, int D, int HW, int K,
                                float *cluster_size, float *vectors_sum, void *stream)
{
    const char *fn = "dvq_ema_accumulate_nchw_x16";
    if (int rc = check_x16_dtype(fn, dtype)) return rc;
    return ema_accumulate_nchw(fn, dtype, z, codes, B, D, HW, K, cluster_size, vectors_sum, stream);
}

// the per-code sums in the fixed order of dvq.h (code_sums_det.hip): codebook == nullptr the statistics, else the codebook gradient
static int code_sums_det(const char *fn, const void *z, int dtype, const float *codebook, const int64_t *codes, const float *mask,
                         const float *g_loss, float coef_scale, int B, int D, int HW, int K, float *count, float *out, void *ws,
                         size_t ws_bytes, void *stream)
{
    if (B <= 0 || D <= 0 || HW <= 0 || K <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (D % 4 != 0) { dvq_set_error("%s: D=%d must be a multiple of 4", fn, D); return DVQ_EUNSUPPORTED; }
    if (K > DVQ_DET_MAX_K) { dvq_set_error("%s: K=%d > %d (the 16-bit code fields of the sorted tile)", fn, K, DVQ_DET_MAX_K); return DVQ_EUNSUPPORTED; }
    const size_t N = (size_t)B * HW;
    if (int rc = check_size(fn, N, true, (size_t)D)) return rc;
    if ((((uintptr_t)z) & (dtype != 0 ? 1 : 3)) != 0 || (((uintptr_t)out | (uintptr_t)codebook) & 15) != 0) {
        dvq_set_error("%s: z must be aligned to its element, the [K, D] arrays to 16 bytes", fn); return DVQ_EINVAL;
    }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_code_sums_det_ws_bytes((long)N, D, K), true)) return rc;
    return hip_rc(dvq_launch_code_sums_det(z, dtype, codebook, (const long long *)codes, mask, g_loss, coef_scale, D, HW, (long)N, K, count,
                                           out, ws, (hipStream_t)stream), fn);
}

size_t dvq_code_sums_det_workspace_bytes(int B, int D, int HW, int K)
{
    if (B <= 0 || D <= 0 || HW <= 0 || K <= 0 || D % 4 != 0 || K > DVQ_DET_MAX_K || (size_t)B * HW >= ((size_t)1 << 31)) return 0;
    return dvq_code_sums_det_ws_bytes((long)B * HW, D, K);
}

int dvq_code_sums_det(const void *z, int dtype, const int64_t *codes, int B, int D, int HW, int K, float *cluster_size,
                      float *vectors_sum, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_code_sums_det";
    if (!z || !codes || !cluster_size || !vectors_sum) return null_pointer(fn);
    if (dtype != 0) { if (int rc = check_x16_dtype(fn, dtype)) return rc; }
    return code_sums_det(fn, z, dtype, nullptr, codes, nullptr, nullptr, 0.0f, B, D, HW, K, cluster_size, vectors_sum, ws, ws_bytes, stream);
}

size_t dvq_vq_backward_codebook_det_workspace_bytes(int B, int D, int HW, int K)
{
    return dvq_code_sums_det_workspace_bytes(B, D, HW, K);
}

int dvq_vq_backward_codebook_det_f32(const float *z, const float *codebook, const int64_t *codes, const float *mask,
                                     const float *g_loss, float coef_scale, int B, int D, int HW, int K, float *g_weight,
                                     void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_vq_backward_codebook_det_f32";
    if (!z || !codebook || !codes || !g_loss || !g_weight) return null_pointer(fn);
    return code_sums_det(fn, z, 0, codebook, codes, mask, g_loss, coef_scale, B, D, HW, K, nullptr, g_weight, ws, ws_bytes, stream);
}

int dvq_code_stats_f32(const int64_t *codes, int64_t N, int K, int64_t *counts, int64_t *n_used, float *perplexity, float *onehot,
                       void *stream)
{
    if (!counts || !n_used || !perplexity || (!codes && N > 0)) return null_pointer("dvq_code_stats_f32");
    if (K < 1 || N < 0) { dvq_set_error("dvq_code_stats_f32: K=%d N=%lld (K >= 1, N >= 0)", K, (long long)N); return DVQ_EINVAL; }
    if (K >= (1 << 20)) { dvq_set_error("dvq_code_stats_f32: K=%d (K < 2^20)", K); return DVQ_EUNSUPPORTED; }
    return hip_rc(dvq_launch_code_stats((const long long *)codes, (long)N, K, (long long *)counts, (long long *)n_used, perplexity, onehot,
                                        (hipStream_t)stream), "code_stats");
}

int dvq_code_stats_grain_f32(const int64_t *codes, const int64_t *grain, int B, int H, int W, int hc, int wc, int G, int K,
                             int64_t *counts, int64_t *n_tokens, int64_t *n_used, float *perplexity, void *stream)
{
    const char *fn = "dvq_code_stats_grain_f32";
    if (!codes || !grain || !counts || !n_tokens || !n_used || !perplexity) return null_pointer(fn);
    if (B < 1 || hc < 1 || wc < 1 || K < 1 || (G != 2 && G != 3)) { dvq_set_error("%s: B=%d hc=%d wc=%d K=%d G=%d (sizes >= 1, G 2 or 3)", fn, B, hc, wc, K, G); return DVQ_EINVAL; }
    const int S = 1 << (G - 1);
    if (hc > (1 << 20) || wc > (1 << 20) || H != hc * S || W != wc * S) {
        dvq_set_error("%s: codes %d x %d against a %d x %d grain map: G=%d needs exactly %d x the cells", fn, H, W, hc, wc, G, S); return DVQ_EINVAL;
    }
    if (K >= (1 << 20) || (int64_t)B * H * W >= ((int64_t)1 << 31)) { dvq_set_error("%s: K=%d B*H*W=%lld (K < 2^20, B*H*W < 2^31)", fn, K, (long long)B * H * W); return DVQ_EUNSUPPORTED; }
    return hip_rc(dvq_launch_code_stats_grain((const long long *)codes, (const long long *)grain, B, H, W, hc, wc, G, K, (long long *)counts,
                                              (long long *)n_tokens, (long long *)n_used, perplexity, (hipStream_t)stream), "code_stats_grain");
}

int dvq_restart_pick_i64(uint64_t seed, int64_t n, int k, int64_t *out, void *stream)
{
    if (!out) return null_pointer("dvq_restart_pick_i64");
    if (k < 1 || k > 2048 || n < 16 * (int64_t)k || n > 0xFFFFFFFFll) {
        dvq_set_error("dvq_restart_pick_i64: k=%d n=%lld (1 <= k <= 2048, 16 k <= n < 2^32)", k, (long long)n); return DVQ_EUNSUPPORTED;
    }
    return hip_rc(dvq_launch_restart_pick((unsigned long long)seed, (long long)n, k, (long long *)out, (hipStream_t)stream), "restart_pick");
}

int dvq_ema_update_f32(const float *stats_sum, const float *stats_count, float decay, float eps, int K, int D,
                       const float *cluster_size_ema, float *cluster_size_out, float *embed_ema, float *weight,
                       int restart, const float *restart_rows, const float *z, int B, int HW, const int64_t *pick, void *stream)
{
    if (!stats_sum || !stats_count || !cluster_size_ema || !cluster_size_out || !embed_ema || !weight) return null_pointer("dvq_ema_update_f32");
    if (K <= 0 || D <= 0) { dvq_set_error("dvq_ema_update_f32: sizes must be positive"); return DVQ_EINVAL; }
    if (cluster_size_out == cluster_size_ema) { dvq_set_error("dvq_ema_update_f32: cluster_size_out must not alias cluster_size_ema (every workgroup sums the OLD counts)"); return DVQ_EINVAL; }
    if (restart < 0 || restart > 2) { dvq_set_error("dvq_ema_update_f32: restart must be 0, 1 or 2"); return DVQ_EINVAL; }
    if (restart == 1 && !restart_rows) { dvq_set_error("dvq_ema_update_f32: restart = 1 needs restart_rows"); return DVQ_EINVAL; }
    if (restart == 2 && (!z || !pick || B <= 0 || HW <= 0)) { dvq_set_error("dvq_ema_update_f32: restart = 2 needs z [B, D, HW] and pick [K]"); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_ema_update(stats_sum, stats_count, decay, eps, K, D, cluster_size_ema, cluster_size_out, embed_ema, weight,
                                        restart, restart_rows, z, HW, (const long long *)pick, (hipStream_t)stream), "ema_update");
}

size_t dvq_router_gate_workspace_bytes(int num_branches, int B, int C, int hc, int wc, int num_groups, int hidden)
{
    if (num_branches < 2 || num_branches > 3 || B <= 0 || C <= 0 || hc <= 0 || wc <= 0 || num_groups < 0 || hidden < 0) return 0;
    // a shape whose feature tile and output-layer rows the direct form cannot hold (dvq_router_gate_f32 refuses it in words)
    if ((num_groups == 0 || C % num_groups == 0) &&
        dvq_router_gate_lds_bytes(num_branches, C, hc, wc, num_groups, hidden > 0 ? hidden : 32, hidden > 0) > DVQ_GATE_LDS_MAX) return 0;
    return dvq_router_gate_ws_bytes(num_branches, B, C, hc, wc, num_groups, hidden > 0 ? hidden : 32);
}

size_t dvq_router_gate_prep_bytes(int num_branches, int C, int hidden)
{
    if (num_branches < 2 || num_branches > 3 || C <= 0 || hidden <= 0) return 0;
    return dvq_router_gate_prep_bytes_impl(num_branches, C, hidden);
}

int dvq_router_gate_prepare_f32(const float *w1, int nb, int C, int hidden, void *w1_prep, size_t w1_prep_bytes, void *stream)
{
    const char *fn = "dvq_router_gate_prepare_f32";
    if (nb != 2 && nb != 3) { dvq_set_error("%s: num_branches=%d (2 or 3)", fn, nb); return DVQ_EINVAL; }
    if (!w1 || !w1_prep || C <= 0 || hidden <= 0) { dvq_set_error("%s: null pointer or non-positive size", fn); return DVQ_EINVAL; }
    if (C % 8 != 0 || nb * C > 1280) { dvq_set_error("%s: C=%d unsupported (C %% 8 == 0, num_branches*C <= 1280)", fn, C); return DVQ_EUNSUPPORTED; }
    if (w1_prep_bytes < dvq_router_gate_prep_bytes(nb, C, hidden)) { dvq_set_error("%s: buffer %zu < %zu bytes", fn, w1_prep_bytes, dvq_router_gate_prep_bytes(nb, C, hidden)); return DVQ_EWORKSPACE; }
    if (((uintptr_t)w1_prep & 255) != 0) { dvq_set_error("%s: buffer must be 256-byte aligned", fn); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_router_gate_prepare(w1, nb, C, hidden, w1_prep, (hipStream_t)stream), "router_gate_prepare");
}

int dvq_router_gate_prepare_norm_f32(int nb, int C, int hidden, const float *gn_w_coarse, const float *gn_b_coarse,
                                     const float *gn_w_median, const float *gn_b_median,
                                     const float *gn_w_fine, const float *gn_b_fine, void *w1_prep, size_t w1_prep_bytes, void *stream)
{
    const char *fn = "dvq_router_gate_prepare_norm_f32";
    if (nb != 2 && nb != 3) { dvq_set_error("%s: num_branches=%d (2 or 3)", fn, nb); return DVQ_EINVAL; }
    if (!w1_prep || !gn_w_coarse || !gn_b_coarse || !gn_w_fine || !gn_b_fine || (nb == 3 && (!gn_w_median || !gn_b_median)) || C <= 0 || hidden <= 0) {
        dvq_set_error("%s: null pointer or non-positive size", fn); return DVQ_EINVAL;
    }
    if (w1_prep_bytes < dvq_router_gate_prep_bytes(nb, C, hidden)) { dvq_set_error("%s: buffer %zu < %zu bytes", fn, w1_prep_bytes, dvq_router_gate_prep_bytes(nb, C, hidden)); return DVQ_EWORKSPACE; }
    const float *w[3] = {gn_w_coarse, nb == 3 ? gn_w_median : gn_w_fine, gn_w_fine};
    const float *b[3] = {gn_b_coarse, nb == 3 ? gn_b_median : gn_b_fine, gn_b_fine};
    return hip_rc(dvq_launch_router_gate_prepare_norm(w, b, nb, C, hidden, w1_prep, (hipStream_t)stream), fn);
}

int dvq_router_gate_f32(int nb, const void *h_coarse, const void *h_median, const void *h_fine,
                        int B, int C, int hc, int wc, int num_groups, float eps,
                        const float *gn_w_coarse, const float *gn_b_coarse,
                        const float *gn_w_median, const float *gn_b_median,
                        const float *gn_w_fine, const float *gn_b_fine,
                        const float *w1, const float *b1, const float *w2, const float *b2,
                        int hidden, int activation_arg, const void *w1_prep, float *gate, void *ws, size_t ws_bytes,
                        void *stream)
{
    const char *fn = "dvq_router_gate_f32";
    const int activation = enum_of(activation_arg), xt = features_of(activation_arg);    // DVQ_FEATURES(dtype): 16-bit branches
    const int nhwc = layout_of(activation_arg);                                          // DVQ_NHWC: channels_last branches
    if (nb != 2 && nb != 3) { dvq_set_error("%s: num_branches=%d (2 or 3)", fn, nb); return DVQ_EINVAL; }
    if (!h_coarse || !h_fine || !w2 || !b2 || !gate) return null_pointer(fn);
    if ((nb == 3) != (h_median != nullptr)) { dvq_set_error("%s: h_median must be given exactly when num_branches == 3", fn); return DVQ_EINVAL; }
    if (B <= 0 || C <= 0 || hc <= 0 || wc <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (activation != DVQ_ACT_NONE && activation != DVQ_ACT_SILU && activation != DVQ_ACT_RELU) { dvq_set_error("%s: unknown activation %d", fn, activation); return DVQ_EINVAL; }
    if (int rc = check_flag_bits(fn, activation_arg)) return rc;
    if (int rc = check_features(fn, xt)) return rc;
    // channels_last branches: the pooling pass takes the piece width the actual alignment allows, down to one element
    if (nhwc && (((uintptr_t)h_coarse | (uintptr_t)h_median | (uintptr_t)h_fine) & (xt != 0 ? 1 : 3)) != 0) {
        dvq_set_error("%s: DVQ_NHWC features must be aligned to their element size (%d bytes)", fn, xt != 0 ? 2 : 4); return DVQ_EINVAL;
    }
    // the pooling pass reads four 2-byte elements with one 8-byte load
    if (!nhwc && xt != 0 && (((uintptr_t)h_coarse | (uintptr_t)h_median | (uintptr_t)h_fine) & 7) != 0) { dvq_set_error("%s: 16-bit features must be 8-byte aligned", fn); return DVQ_EINVAL; }
    if (activation != DVQ_ACT_NONE && (!w1 || !b1 || hidden <= 0)) { dvq_set_error("%s: hidden layer requested without w1 / b1 / hidden", fn); return DVQ_EINVAL; }
    if (num_groups < 0 || (num_groups > 0 && C % num_groups != 0)) { dvq_set_error("%s: C=%d is not divisible by num_groups=%d", fn, C, num_groups); return DVQ_EINVAL; }
    if (num_groups > 0 && (!gn_w_coarse || !gn_b_coarse || !gn_w_fine || !gn_b_fine || (nb == 3 && (!gn_w_median || !gn_b_median)))) {
        dvq_set_error("%s: GroupNorm affine parameters missing", fn); return DVQ_EINVAL;
    }
    if (C % 8 != 0 || nb * C > 1280) { dvq_set_error("%s: C=%d unsupported (C %% 8 == 0, num_branches*C <= 1280)", fn, C); return DVQ_EUNSUPPORTED; }
    if (num_groups > 0 && ((size_t)(C / num_groups) * hc * wc) % 4 != 0) { dvq_set_error("%s: group size not a multiple of 4 floats", fn); return DVQ_EUNSUPPORTED; }
    const int hid = activation == DVQ_ACT_NONE ? 32 : hidden;
    if (const size_t lds = dvq_router_gate_lds_bytes(nb, C, hc, wc, num_groups, hid, activation); lds > DVQ_GATE_LDS_MAX) {
        dvq_set_error("%s: num_branches=%d C=%d hidden=%d needs %zu bytes of LDS, %d available (128 * (num_branches*C rounded up to 16) + 4 * (1 + num_branches) * hidden)",
                      fn, nb, C, hid, lds, DVQ_GATE_LDS_MAX);
        return DVQ_EUNSUPPORTED;
    }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_router_gate_ws_bytes(nb, B, C, hc, wc, num_groups, hidden > 0 ? hidden : 32))) return rc;
    const void *h[3];
    const float *gw[3], *gb[3];
    if (nb == 2) {
        h[0] = h_coarse; h[1] = h_fine; h[2] = nullptr;
        gw[0] = gn_w_coarse; gw[1] = gn_w_fine; gw[2] = nullptr;
        gb[0] = gn_b_coarse; gb[1] = gn_b_fine; gb[2] = nullptr;
    } else {
        h[0] = h_coarse; h[1] = h_median; h[2] = h_fine;
        gw[0] = gn_w_coarse; gw[1] = gn_w_median; gw[2] = gn_w_fine;
        gb[0] = gn_b_coarse; gb[1] = gn_b_median; gb[2] = gn_b_fine;
    }
    return hip_rc(dvq_launch_router_gate(nb, h, xt, nhwc, gw, gb, B, C, hc, wc, num_groups, eps, w1, b1, w2, b2,
                                         hid, activation, w1_prep, gate, ws, (hipStream_t)stream), "router_gate");
}

// shared argument checks of the training-mode routing tail; fills the branch / parameter slots of *a
static int route_train_args(const char *fn, DvqRouteTrain *a, int nb, const float *h_coarse, const float *h_median, const float *h_fine,
                            int B, int C, int hc, int wc, int num_groups, float eps,
                            const float *gn_w_coarse, const float *gn_b_coarse, const float *gn_w_median, const float *gn_b_median,
                            const float *gn_w_fine, const float *gn_b_fine, const float *w1, const float *b1, const float *w2,
                            const float *b2, int hidden, int activation, const float *gumbels, float tau, void *ws, size_t ws_bytes)
{
    if (nb != 2 && nb != 3) { dvq_set_error("%s: num_branches=%d (2 or 3)", fn, nb); return DVQ_EINVAL; }
    if (!h_coarse || !h_fine || !w2 || !b2) return null_pointer(fn);
    if ((nb == 3) != (h_median != nullptr)) { dvq_set_error("%s: h_median must be given exactly when num_branches == 3", fn); return DVQ_EINVAL; }
    if (B <= 0 || C <= 0 || hc <= 0 || wc <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (activation != DVQ_ACT_NONE && activation != DVQ_ACT_SILU && activation != DVQ_ACT_RELU) { dvq_set_error("%s: unknown activation %d", fn, activation); return DVQ_EINVAL; }
    if (activation != DVQ_ACT_NONE && (!w1 || !b1 || hidden <= 0)) { dvq_set_error("%s: hidden layer requested without w1 / b1 / hidden", fn); return DVQ_EINVAL; }
    if (activation == DVQ_ACT_NONE && hidden != 0) { dvq_set_error("%s: hidden must be 0 with DVQ_ACT_NONE", fn); return DVQ_EINVAL; }
    if (num_groups < 0 || (num_groups > 0 && C % num_groups != 0)) { dvq_set_error("%s: C=%d is not divisible by num_groups=%d", fn, C, num_groups); return DVQ_EINVAL; }
    if (num_groups > 0 && (!gn_w_coarse || !gn_b_coarse || !gn_w_fine || !gn_b_fine || (nb == 3 && (!gn_w_median || !gn_b_median)))) {
        dvq_set_error("%s: GroupNorm affine parameters missing", fn); return DVQ_EINVAL;
    }
    if (!(tau > 0.0f)) { dvq_set_error("%s: tau must be positive", fn); return DVQ_EINVAL; }
    const int S = nb == 2 ? 2 : 4;
    if (C % 8 != 0 || nb * C > 1280 || hidden > 1280) { dvq_set_error("%s: C=%d hidden=%d unsupported (C %% 8 == 0, num_branches*C <= 1280, hidden <= 1280)", fn, C, hidden); return DVQ_EUNSUPPORTED; }
    if ((long)S * wc > 4096 || (double)B * C * S * hc * S * wc >= 2147483648.0) { dvq_set_error("%s: grid %dx%d x B=%d too large", fn, hc, wc, B); return DVQ_EUNSUPPORTED; }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_route_train_ws_bytes(nb, B, C, hc, wc, num_groups, hidden))) return rc;
    *a = DvqRouteTrain{};
    a->nb = nb; a->B = B; a->C = C; a->hc = hc; a->wc = wc; a->groups = num_groups; a->eps = eps;
    const float *hs[3] = {h_coarse, nb == 3 ? h_median : h_fine, h_fine};
    const float *gw[3] = {gn_w_coarse, nb == 3 ? gn_w_median : gn_w_fine, gn_w_fine};
    const float *gb[3] = {gn_b_coarse, nb == 3 ? gn_b_median : gn_b_fine, gn_b_fine};
    for (int i = 0; i < 3; ++i) { a->h[i] = i < nb ? hs[i] : nullptr; a->gn_w[i] = i < nb ? gw[i] : nullptr; a->gn_b[i] = i < nb ? gb[i] : nullptr; }
    a->w1 = w1; a->b1 = b1; a->w2 = w2; a->b2 = b2;
    a->hid = activation == DVQ_ACT_NONE ? 0 : hidden;
    a->act = activation;
    a->gumbels = gumbels; a->tau = tau; a->ws = ws;
    return DVQ_OK;
}

size_t dvq_route_train_workspace_bytes(int nb, int B, int C, int hc, int wc, int num_groups, int hidden)
{
    if ((nb != 2 && nb != 3) || B <= 0 || C <= 0 || hc <= 0 || wc <= 0 || num_groups < 0 || hidden < 0) return 0;
    if (C % 8 != 0 || nb * C > 1280 || hidden > 1280) return 0;
    return dvq_route_train_ws_bytes(nb, B, C, hc, wc, num_groups, hidden);
}

int dvq_route_train_forward_f32(int nb, const float *h_coarse, const float *h_median, const float *h_fine,
                                int B, int C, int hc, int wc, int num_groups, float eps,
                                const float *gn_w_coarse, const float *gn_b_coarse,
                                const float *gn_w_median, const float *gn_b_median,
                                const float *gn_w_fine, const float *gn_b_fine,
                                const float *w1, const float *b1, const float *w2, const float *b2,
                                int hidden, int activation, const float *gumbels, float tau,
                                float *h_out, int64_t *indices, float *codebook_mask, float *gate,
                                void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_route_train_forward_f32";
    DvqRouteTrain a;
    const int rc = route_train_args(fn, &a, nb, h_coarse, h_median, h_fine, B, C, hc, wc, num_groups, eps, gn_w_coarse, gn_b_coarse,
                                    gn_w_median, gn_b_median, gn_w_fine, gn_b_fine, w1, b1, w2, b2, hidden, activation, gumbels, tau,
                                    ws, ws_bytes);
    if (rc != DVQ_OK) return rc;
    if (!h_out || !indices || !codebook_mask || !gate) { dvq_set_error("%s: null output pointer", fn); return DVQ_EINVAL; }
    a.h_out = h_out; a.indices = (long long *)indices; a.cmask = codebook_mask; a.gate = gate;
    return hip_rc(dvq_launch_route_train_fwd(&a, (hipStream_t)stream), "route_train_forward");
}

int dvq_route_train_backward_f32(int nb, const float *h_coarse, const float *h_median, const float *h_fine,
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
                                 float *dw1, float *db1, float *dw2, float *db2, void *stream)
{
    const char *fn = "dvq_route_train_backward_f32";
    DvqRouteTrain a;
    const int rc = route_train_args(fn, &a, nb, h_coarse, h_median, h_fine, B, C, hc, wc, num_groups, eps, gn_w_coarse, gn_b_coarse,
                                    gn_w_median, gn_b_median, gn_w_fine, gn_b_fine, w1, b1, w2, b2, hidden, activation, gumbels, tau,
                                    ws, ws_bytes);
    if (rc != DVQ_OK) return rc;
    if (!dh_coarse || !dh_fine || (nb == 3 && !dh_median) || !dw2 || !db2 || (a.hid > 0 && (!dw1 || !db1))) {
        dvq_set_error("%s: null output pointer", fn); return DVQ_EINVAL;
    }
    if (num_groups > 0 && (!dgn_w_coarse || !dgn_b_coarse || !dgn_w_fine || !dgn_b_fine || (nb == 3 && (!dgn_w_median || !dgn_b_median)))) {
        dvq_set_error("%s: GroupNorm gradient outputs missing", fn); return DVQ_EINVAL;
    }
    a.g_out = g_out; a.g_gate = g_gate;
    float *dh[3] = {dh_coarse, nb == 3 ? dh_median : dh_fine, dh_fine};
    float *dw[3] = {dgn_w_coarse, nb == 3 ? dgn_w_median : dgn_w_fine, dgn_w_fine};
    float *db[3] = {dgn_b_coarse, nb == 3 ? dgn_b_median : dgn_b_fine, dgn_b_fine};
    for (int i = 0; i < 3; ++i) { a.dh[i] = i < nb ? dh[i] : nullptr; a.dgn_w[i] = i < nb ? dw[i] : nullptr; a.dgn_b[i] = i < nb ? db[i] : nullptr; }
    a.dw1 = dw1; a.db1 = db1; a.dw2 = dw2; a.db2 = db2;
    return hip_rc(dvq_launch_route_train_bwd(&a, (hipStream_t)stream), "route_train_backward");
}

int dvq_entropy_map_f32(const float *images, int B, int H, int W, int patch, float *out, void *stream)
{
    if (!images || !out) return null_pointer("dvq_entropy_map_f32");
    if (B <= 0 || H <= 0 || W <= 0) { dvq_set_error("dvq_entropy_map_f32: sizes must be positive"); return DVQ_EINVAL; }
    if (patch != 16 || H % 16 != 0 || W % 16 != 0) { dvq_set_error("dvq_entropy_map_f32: patch=%d H=%d W=%d (patch 16, H and W multiples of 16)", patch, H, W); return DVQ_EUNSUPPORTED; }
    if ((long)B * (H / 16) * (W / 16) >= (1L << 30)) { dvq_set_error("dvq_entropy_map_f32: %ld patches (at most 2^30 per call)", (long)B * (H / 16) * (W / 16)); return DVQ_EUNSUPPORTED; }
    return hip_rc(dvq_launch_entropy_map(images, B, H, W, out, (hipStream_t)stream), "entropy_map");
}

static int perm_dims_ok(const char *fn, int B, int hc, int wc)
{
    if (B <= 0 || hc <= 0 || wc <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if ((long)hc * wc > dvq_permute_max_cells()) { dvq_set_error("%s: hc*wc=%ld exceeds %d coarse cells", fn, (long)hc * wc, dvq_permute_max_cells()); return DVQ_EUNSUPPORTED; }
    return DVQ_OK;
}

int dvq_permute_dual_count_i64(const int64_t *grain, int B, int hc, int wc, int32_t *counts, int32_t *maxes,
                               void *stream)
{
    if (!grain || !counts || !maxes) return null_pointer("dvq_permute_dual_count_i64");
    int rc = perm_dims_ok("dvq_permute_dual_count_i64", B, hc, wc);
    if (rc) return rc;
    return hip_rc(dvq_launch_permute_count((const long long *)grain, B, hc * wc, counts, maxes, (hipStream_t)stream), "permute_count");
}

int dvq_permute_dual_forward_i64(const int64_t *codes, const int64_t *grain, int B, int hc, int wc,
                                 int order, int Lc, int Lf, const int64_t *special,
                                 int64_t *coarse_content, int64_t *coarse_position, int64_t *coarse_segment,
                                 int64_t *fine_content, int64_t *fine_position, int64_t *fine_segment,
                                 void *stream)
{
    if (!codes || !grain || !special || !coarse_content || !coarse_position || !coarse_segment || !fine_content ||
        !fine_position || !fine_segment) return null_pointer("dvq_permute_dual_forward_i64");
    int rc = perm_dims_ok("dvq_permute_dual_forward_i64", B, hc, wc);
    if (rc) return rc;
    if (order != 0 && order != 1) { dvq_set_error("dvq_permute_dual_forward_i64: order %d (0 region-first, 1 row-first)", order); return DVQ_EINVAL; }
    if (Lc <= 0 || Lf <= 0) { dvq_set_error("dvq_permute_dual_forward_i64: Lc, Lf must be positive"); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_permute_forward((const long long *)codes, (const long long *)grain, B, hc, wc, order, Lc, Lf,
                                             (const long long *)special, (long long *)coarse_content,
                                             (long long *)coarse_position, (long long *)coarse_segment,
                                             (long long *)fine_content, (long long *)fine_position,
                                             (long long *)fine_segment, (hipStream_t)stream), "permute_forward");
}

int dvq_permute_dual_backward_i64(const int64_t *coarse_content, const int64_t *fine_content,
                                  const int64_t *coarse_position, const int64_t *fine_position,
                                  int B, int Lc, int Lf, int hc, int wc,
                                  int64_t coarse_position_eos, int64_t fine_position_eos,
                                  int64_t *target, void *stream)
{
    if (!coarse_content || !fine_content || !coarse_position || !fine_position || !target) return null_pointer("dvq_permute_dual_backward_i64");
    int rc = perm_dims_ok("dvq_permute_dual_backward_i64", B, hc, wc);
    if (rc) return rc;
    if (Lc <= 0 || Lf <= 0) { dvq_set_error("dvq_permute_dual_backward_i64: Lc, Lf must be positive"); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_permute_backward((const long long *)coarse_content, (const long long *)fine_content,
                                              (const long long *)coarse_position, (const long long *)fine_position,
                                              B, Lc, Lf, hc, wc, coarse_position_eos, fine_position_eos,
                                              (long long *)target, (hipStream_t)stream), "permute_backward");
}

size_t dvq_qconv_prep_bytes(int D) { return dim_ok(D) ? dvq_qconv_prep_bytes_impl(D) : 0; }

int dvq_qconv_prepare_f32(const float *weight, const float *bias, int D, void *prep, size_t prep_bytes, void *stream)
{
    if (!weight || !prep) return null_pointer("dvq_qconv_prepare_f32");
    if (int rc = check_width("dvq_qconv_prepare_f32", D)) return rc;
    if (int rc = check_prep_buffer("dvq_qconv_prepare_f32", prep, prep_bytes, dvq_qconv_prep_bytes(D))) return rc;
    return hip_rc(dvq_launch_qconv_prep(weight, bias, D, prep, (hipStream_t)stream), "qconv_prep");
}

int dvq_qconv_f32(const float *x, const void *prep, int B, int D, int HW, float *h, void *stream)
{
    if (!x || !prep || !h) return null_pointer("dvq_qconv_f32");
    if (B <= 0 || HW <= 0) { dvq_set_error("dvq_qconv_f32: sizes must be positive"); return DVQ_EINVAL; }
    if (int rc = check_width("dvq_qconv_f32", D)) return rc;
    if (int rc = check_size("dvq_qconv_f32", (size_t)B * HW, true)) return rc;
    return hip_rc(dvq_launch_qconv(x, nullptr, prep, D, HW, (long)B * HW, h, (hipStream_t)stream), "qconv");
}

int dvq_qconv_select_f32(int num_branches, const void *gate, int gate_kind, float threshold,
                         const float *h_coarse, const float *h_median, const float *h_fine, const void *prep,
                         int B, int D, int hc, int wc, float *h, int64_t *indices, float *cmask, int64_t *gate_out,
                         void *stream)
{
    const char *fn = "dvq_qconv_select_f32";
    if (num_branches != 2 && num_branches != 3) { dvq_set_error("%s: num_branches=%d (2 or 3)", fn, num_branches); return DVQ_EINVAL; }
    if (!gate || !h_coarse || !h_fine || !prep || !h || !indices || !cmask || (num_branches == 3 && !h_median)) {
        return null_pointer(fn);
    }
    if (B <= 0 || hc <= 0 || wc <= 0) { dvq_set_error("%s: sizes must be positive", fn); return DVQ_EINVAL; }
    if (gate_kind != DVQ_GATE_F32 && gate_kind != DVQ_GATE_I64 && gate_kind != DVQ_GATE_ENTROPY) { dvq_set_error("%s: gate_kind %d", fn, gate_kind); return DVQ_EINVAL; }
    if (gate_kind == DVQ_GATE_ENTROPY && num_branches != 2) { dvq_set_error("%s: the entropy gate is a dual-granularity router", fn); return DVQ_EINVAL; }
    if (int rc = check_width(fn, D)) return rc;
    const int SC = (num_branches == 2) ? 2 : 4;
    const long N = (long)B * SC * hc * SC * wc;
    if (int rc = check_size(fn, (size_t)N, true)) return rc;
    DvqRouted rv{};
    rv.G = num_branches; rv.B = B; rv.D = D; rv.hc = hc; rv.wc = wc; rv.Wout = SC * wc; rv.HWout = SC * hc * SC * wc;
    rv.gate = gate; rv.gate_mode = (gate_kind == DVQ_GATE_ENTROPY) ? 2 : (gate_kind == DVQ_GATE_I64 ? 1 : 0);
    rv.thr = threshold; rv.indices = (const long long *)indices;
    rv.indices_out = (long long *)indices; rv.cmask_out = cmask; rv.gate_out = (long long *)gate_out;
    if (num_branches == 2) {
        rv.src[0] = h_coarse; rv.src[1] = h_fine; rv.sub[0] = 1; rv.sub[1] = 2; rv.sub[2] = 1; rv.rep[0] = 2; rv.rep[1] = 1; rv.rep[2] = 1;
    } else {
        rv.src[0] = h_coarse; rv.src[1] = h_median; rv.src[2] = h_fine;
        rv.sub[0] = 1; rv.sub[1] = 2; rv.sub[2] = 4; rv.rep[0] = 4; rv.rep[1] = 2; rv.rep[2] = 1;
    }
    return hip_rc(dvq_launch_qconv(nullptr, &rv, prep, D, rv.HWout, N, h, (hipStream_t)stream), fn);
}

int dvq_debug_filter_scores_f32(const float *tokens, int n, const void *prep, int D, int K, float *scores,
                                float *threshold, float *xn, float *scale, void *stream)
{
    if (!tokens || !prep || !scores || !threshold || !xn) return null_pointer("dvq_debug_filter_scores_f32");
    if (n <= 0 || K <= 0) { dvq_set_error("dvq_debug_filter_scores_f32: n, K must be positive"); return DVQ_EINVAL; }
    if (!dim_ok(D)) { dvq_set_error("dvq_debug_filter_scores_f32: D=%d unsupported", D); return DVQ_EUNSUPPORTED; }
    return hip_rc(dvq_launch_filter_scores_debug(tokens, n, prep, D, K, scores, threshold, xn, scale, (hipStream_t)stream),
                  "filter_scores_debug");
}

int dvq_debug_fold_scores_f32(const float *tokens, int n, const void *fold_prep, int D, int K, float *scores,
                              float *threshold, float *xn, float *scale, void *stream)
{
    if (!tokens || !fold_prep || !scores || !threshold || !xn) return null_pointer("dvq_debug_fold_scores_f32");
    if (n <= 0 || K <= 0) { dvq_set_error("dvq_debug_fold_scores_f32: n, K must be positive"); return DVQ_EINVAL; }
    if (!dim_ok(D)) { dvq_set_error("dvq_debug_fold_scores_f32: D=%d unsupported", D); return DVQ_EUNSUPPORTED; }
    return hip_rc(dvq_launch_filter_scores_debug(tokens, n, fold_prep, D, K, scores, threshold, xn, scale, (hipStream_t)stream, 1),
                  "fold_scores_debug");
}

size_t dvq_exchange_bytes(int64_t codes_per_image, int64_t grain_per_image, int b_max, int num_codes)
{
    if (codes_per_image <= 0 || grain_per_image < 0 || b_max <= 0 || num_codes <= 0) return 0;
    return dvq_xch_bytes((long)codes_per_image, (long)grain_per_image, b_max, num_codes);
}

int dvq_exchange_pack(const int64_t *codes, const int64_t *grain, const float *loss, double numel, int b_local,
                      int b_max, int64_t codes_per_image, int64_t grain_per_image, int num_codes, void *buf,
                      void *stream)
{
    // an empty shard (b_local == 0: global_batch < world) has nothing to point at: its codes and grain may be null
    if ((!codes && b_local != 0) || !buf) return null_pointer("dvq_exchange_pack");
    if (b_local < 0 || b_max <= 0 || b_local > b_max || codes_per_image <= 0 || grain_per_image < 0 || num_codes <= 0) {
        dvq_set_error("dvq_exchange_pack: bad sizes"); return DVQ_EINVAL;
    }
    if (grain_per_image > 0 && !grain && b_local != 0) { dvq_set_error("dvq_exchange_pack: null grain"); return DVQ_EINVAL; }
    if (((uintptr_t)buf & 7) != 0) { dvq_set_error("dvq_exchange_pack: buffer must be 8-byte aligned"); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_xch_pack((const long long *)codes, grain_per_image > 0 ? (const long long *)grain : nullptr,
                                      loss, numel, b_local, b_max, (long)codes_per_image, (long)grain_per_image,
                                      num_codes, buf, (hipStream_t)stream), "exchange_pack");
}

int dvq_exchange_unpack(const void *gathered, int world, int global_batch, int64_t codes_per_image,
                        int64_t grain_per_image, int num_codes, int64_t *codes, int64_t *grain, float *mean,
                        void *stream)
{
    if (!gathered || !codes) return null_pointer("dvq_exchange_unpack");
    if (world <= 0 || global_batch <= 0 || codes_per_image <= 0 || grain_per_image < 0 || num_codes <= 0) {
        dvq_set_error("dvq_exchange_unpack: bad sizes"); return DVQ_EINVAL;
    }
    if (grain_per_image > 0 && !grain) { dvq_set_error("dvq_exchange_unpack: null grain"); return DVQ_EINVAL; }
    if (((uintptr_t)gathered & 7) != 0) {                  // read as shorts, ints and doubles; every rank's slice is a multiple of 8 bytes
        dvq_set_error("dvq_exchange_unpack: buffer must be 8-byte aligned"); return DVQ_EINVAL;
    }
    return hip_rc(dvq_launch_xch_unpack(gathered, world, global_batch, (long)codes_per_image, (long)grain_per_image,
                                        num_codes, (long long *)codes, grain_per_image > 0 ? (long long *)grain : nullptr,
                                        mean, (hipStream_t)stream), "exchange_unpack");
}

// ---- residual quantization (rq.hip) ------------------------------------------------------------------------------------
static bool rq_width_ok(int D) { return D > 0 && D <= 256 && D % 32 == 0; }

static size_t rq_ws_bytes(long N, int D, int depth, int want_grad)
{
    size_t o0, o1, oa, os, tot;
    dvq_rq_layout(N, D, depth, want_grad, &o0, &o1, &oa, &os, &tot);
    return tot;
}

// shared checks of the step / backward / embed geometry: -> DVQ_OK or the error code (message set)
static int rq_geom_check(const char *fn, int B, int h, int w, int rH, int rW, int Dl, int D, int depth)
{
    if (B <= 0 || h <= 0 || w <= 0 || rH <= 0 || rW <= 0 || Dl <= 0 || D <= 0) {
        dvq_set_error("%s: B=%d h=%d w=%d rH=%d rW=%d Dl=%d D=%d must be positive", fn, B, h, w, rH, rW, Dl, D); return DVQ_EINVAL;
    }
    if (depth < 1 || depth > DVQ_RQ_MAX_DEPTH) { dvq_set_error("%s: depth=%d outside [1, %d]", fn, depth, DVQ_RQ_MAX_DEPTH); return DVQ_EINVAL; }
    if ((long)Dl * rH * rW != D) { dvq_set_error("%s: Dl * rH * rW = %d * %d * %d != D = %d", fn, Dl, rH, rW, D); return DVQ_EINVAL; }
    if (!rq_width_ok(D)) { dvq_set_error("%s: D=%d unsupported (a multiple of 32 up to 256: the widths the assign serves)", fn, D); return DVQ_EUNSUPPORTED; }
    if ((long)B * h * w * D >= (1L << 31)) { dvq_set_error("%s: N * D = %ld >= 2^31", fn, (long)B * h * w * D); return DVQ_EUNSUPPORTED; }
    return DVQ_OK;
}

size_t dvq_rq_workspace_bytes(int64_t N, int D, int depth, int want_grad)
{
    if (N <= 0 || !rq_width_ok(D) || N * D >= ((int64_t)1 << 31) || depth < 1 || depth > DVQ_RQ_MAX_DEPTH) return 0;
    return rq_ws_bytes((long)N, D, depth, want_grad ? 1 : 0);
}

size_t dvq_rq_residual_offset(int64_t N, int D, int depth, int i)
{
    if (N <= 0 || !rq_width_ok(D) || N * D >= ((int64_t)1 << 31) || depth < 1 || depth > DVQ_RQ_MAX_DEPTH || i < 1 || i >= depth) return 0;
    size_t o0, o1, oa, os, tot;
    dvq_rq_layout((long)N, D, depth, 0, &o0, &o1, &oa, &os, &tot);
    return ((i - 1) & 1) ? o1 : o0;
}

int dvq_rq_step_f32(const float *x, const float *r, const float *codebook, int K, const int64_t *code,
                    int B, int h, int w, int rH, int rW, int Dl, int D, int i, int depth, int want_grad,
                    int64_t *codes, float *out, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_rq_step_f32";
    if (!x || !r || !codebook || !code || !codes || !out || !ws) return null_pointer(fn);
    if (K <= 0) { dvq_set_error("%s: K=%d must be positive", fn, K); return DVQ_EINVAL; }
    const int rc = rq_geom_check(fn, B, h, w, rH, rW, Dl, D, depth);
    if (rc != DVQ_OK) return rc;
    if (i < 0 || i >= depth) { dvq_set_error("%s: i=%d outside [0, depth=%d)", fn, i, depth); return DVQ_EINVAL; }
    if (int rc = check_ws_aligned(fn, ws)) return rc;
    const long N = (long)B * h * w;
    if (ws_bytes < rq_ws_bytes(N, D, depth, want_grad ? 1 : 0)) {
        dvq_set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, rq_ws_bytes(N, D, depth, want_grad ? 1 : 0)); return DVQ_EWORKSPACE;
    }
    return hip_rc(dvq_launch_rq_step(x, r, codebook, K, (const long long *)code, B, h, w, rH, rW, Dl, i, depth, want_grad ? 1 : 0,
                                     (long long *)codes, out, ws, (hipStream_t)stream), "rq_step");
}

int dvq_rq_loss_f32(int64_t N, int D, int depth, const void *ws, size_t ws_bytes, float *loss, void *stream)
{
    const char *fn = "dvq_rq_loss_f32";
    if (!ws || !loss) return null_pointer(fn);
    if (N <= 0 || depth < 1 || depth > DVQ_RQ_MAX_DEPTH) { dvq_set_error("%s: N=%lld depth=%d out of range", fn, (long long)N, depth); return DVQ_EINVAL; }
    if (!rq_width_ok(D) || N * D >= ((int64_t)1 << 31)) { dvq_set_error("%s: D=%d unsupported", fn, D); return DVQ_EUNSUPPORTED; }
    if (int rc = check_ws_aligned(fn, ws)) return rc;
    if (ws_bytes < rq_ws_bytes((long)N, D, depth, 0)) { dvq_set_error("%s: workspace %zu < %zu bytes", fn, ws_bytes, rq_ws_bytes((long)N, D, depth, 0)); return DVQ_EWORKSPACE; }
    return hip_rc(dvq_launch_rq_loss((long)N, D, depth, ws, loss, (hipStream_t)stream), "rq_loss");
}

int dvq_rq_backward_f32(const float *g_out, const float *g_loss, int B, int h, int w, int rH, int rW, int Dl, int D,
                        int depth, const void *ws, size_t ws_bytes, float *g_x, void *stream)
{
    const char *fn = "dvq_rq_backward_f32";
    if (!ws || !g_x) return null_pointer(fn);
    const int rc = rq_geom_check(fn, B, h, w, rH, rW, Dl, D, depth);
    if (rc != DVQ_OK) return rc;
    if (int rc = check_ws_aligned(fn, ws)) return rc;
    const long N = (long)B * h * w;
    if (ws_bytes < rq_ws_bytes(N, D, depth, 1)) { dvq_set_error("%s: workspace %zu < %zu bytes (the want_grad workspace of the forward)", fn, ws_bytes, rq_ws_bytes(N, D, depth, 1)); return DVQ_EWORKSPACE; }
    return hip_rc(dvq_launch_rq_backward(g_out, g_loss, B, h, w, rH, rW, Dl, depth, ws, g_x, (hipStream_t)stream), "rq_backward");
}

int dvq_rq_embed_code_f32(const float *const *codebooks, const int *K, int depth, const int64_t *codes,
                          int B, int h, int w, int rH, int rW, int Dl, int D, int mode, int j, float *out, void *stream)
{
    const char *fn = "dvq_rq_embed_code_f32";
    if (!codebooks || !K || !codes || !out) return null_pointer(fn);
    const int rc = rq_geom_check(fn, B, h, w, rH, rW, Dl, D, depth);
    if (rc != DVQ_OK) return rc;
    for (int t = 0; t < depth; ++t)
        if (!codebooks[t] || K[t] <= 0) { dvq_set_error("%s: codebook %d is null or K <= 0", fn, t); return DVQ_EINVAL; }
    if (mode != DVQ_RQ_EMBED_SUM && mode != DVQ_RQ_EMBED_SELECT && mode != DVQ_RQ_EMBED_EACH) { dvq_set_error("%s: unknown mode %d", fn, mode); return DVQ_EINVAL; }
    if (j < 0 || j >= depth) { dvq_set_error("%s: j=%d outside [0, depth=%d)", fn, j, depth); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_rq_embed(codebooks, K, depth, (const long long *)codes, B, h, w, rH, rW, Dl, mode, j, out,
                                      (hipStream_t)stream), "rq_embed_code");
}

int dvq_sample_head_f32(const float *logits, int64_t logits_row_stride, int B, int V, float temperature, const int64_t *rules,
                        const int64_t *history, int64_t history_row_stride, int history_len, float *flag, int top_k,
                        float top_p, int sample, const float *q, int64_t *tokens, int64_t tokens_row_stride,
                        float *out_logits, float *out_probs, void *stream)
{
    const char *fn = "dvq_sample_head_f32";
    if (!logits || !rules || !flag || !tokens || (sample && !q) || (history_len > 0 && !history)) {
        return null_pointer(fn);
    }
    if (B <= 0 || V <= 0) { dvq_set_error("%s: B=%d V=%d must be positive", fn, B, V); return DVQ_EINVAL; }
    if (V > dvq_sample_max_vocab()) { dvq_set_error("%s: V=%d exceeds %d", fn, V, dvq_sample_max_vocab()); return DVQ_EUNSUPPORTED; }
    if (!(temperature > 0.0f)) { dvq_set_error("%s: temperature must be > 0", fn); return DVQ_EINVAL; }
    if (top_k < 0 || top_k > V) { dvq_set_error("%s: top_k=%d (0 = off, else 1..V=%d)", fn, top_k, V); return DVQ_EINVAL; }
    if (!(top_p >= 0.0f && top_p <= 1.0f)) { dvq_set_error("%s: top_p outside (0, 1] (0 = off)", fn); return DVQ_EINVAL; }
    if (rules[0] < 0 || rules[0] >= V) { dvq_set_error("%s: pad code %lld outside [0, V=%d)", fn, (long long)rules[0], V); return DVQ_EINVAL; }
    for (int i = 1; i < 7; ++i) {
        const bool range = i == 2 || i == 5;                   // ban_from codes may be V (an empty range)
        if (rules[i] < -1 || rules[i] > (range ? V : V - 1)) {
            dvq_set_error("%s: rule code %d = %lld outside [0, V=%d) (-1 = unused)", fn, i, (long long)rules[i], V); return DVQ_EINVAL;
        }
    }
    if (logits_row_stride < V || tokens_row_stride < 1 || history_len < 0 || (history_len > 0 && history_row_stride < history_len)) {
        dvq_set_error("%s: bad stride / history length", fn); return DVQ_EINVAL;
    }
    return hip_rc(dvq_launch_sample_head(logits, logits_row_stride, B, V, temperature, (const long long *)rules,
                                         (const long long *)history, history_row_stride, history_len, flag,
                                         top_k, top_p, sample, q, (long long *)tokens, tokens_row_stride, out_logits,
                                         out_probs, (hipStream_t)stream), "sample_head");
}

static int transfer_args_ok(const char *fn, const int64_t *coarse_position, int64_t row_stride, int B, int Lc, int hc, int variant)
{
    if (!coarse_position) return null_pointer(fn);
    if (B <= 0 || Lc <= 0 || hc <= 0 || row_stride < Lc) { dvq_set_error("%s: B=%d Lc=%d hc=%d stride=%lld", fn, B, Lc, hc, (long long)row_stride); return DVQ_EINVAL; }
    if ((long)hc * hc > dvq_sample_max_cells()) { dvq_set_error("%s: hc*hc=%ld exceeds %d coarse cells", fn, (long)hc * hc, dvq_sample_max_cells()); return DVQ_EUNSUPPORTED; }
    if (variant != DVQ_TRANSFER_SAMPLED && variant != DVQ_TRANSFER_REMAIN) { dvq_set_error("%s: variant %d", fn, variant); return DVQ_EINVAL; }
    return DVQ_OK;
}

int dvq_sample_transfer_count_i64(const int64_t *coarse_position, int64_t row_stride, int B, int Lc, int hc,
                                  int64_t coarse_position_eos, int variant, int32_t *counts, int32_t *max_count, void *stream)
{
    const char *fn = "dvq_sample_transfer_count_i64";
    int rc = transfer_args_ok(fn, coarse_position, row_stride, B, Lc, hc, variant);
    if (rc) return rc;
    if (!counts || !max_count) return null_pointer(fn);
    return hip_rc(dvq_launch_transfer_count((const long long *)coarse_position, row_stride, B, Lc, hc, coarse_position_eos,
                                            variant, counts, max_count, (hipStream_t)stream), "transfer_count");
}

int dvq_sample_transfer_fill_i64(const int64_t *coarse_position, int64_t row_stride, int B, int Lc, int hc,
                                 int64_t coarse_position_eos, int variant, int order, int sos_mode, int64_t sos_code,
                                 int64_t fine_position_eos, int64_t fine_position_pad, int L, int64_t *out, void *stream)
{
    const char *fn = "dvq_sample_transfer_fill_i64";
    int rc = transfer_args_ok(fn, coarse_position, row_stride, B, Lc, hc, variant);
    if (rc) return rc;
    if (!out) return null_pointer(fn);
    if (order != 0 && order != 1) { dvq_set_error("%s: order %d (0 region-first, 1 row-first)", fn, order); return DVQ_EINVAL; }
    if (sos_mode < DVQ_TRANSFER_SOS_NONE || sos_mode > DVQ_TRANSFER_SOS_COPY) { dvq_set_error("%s: sos_mode %d", fn, sos_mode); return DVQ_EINVAL; }
    if (L < 1) { dvq_set_error("%s: L=%d must be positive", fn, L); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_transfer_fill((const long long *)coarse_position, row_stride, B, Lc, hc, coarse_position_eos,
                                           variant, order, sos_mode, sos_code, fine_position_eos, fine_position_pad, L,
                                           (long long *)out, (hipStream_t)stream), "transfer_fill");
}

#define DVQ_DECODE_MAX_C 1024   // channels of the decode head; also the widest codebook the table kernel keeps in LDS

size_t dvq_decode_table_bytes(int rows, int C)
{
    if (rows <= 0 || C <= 0) return 0;
    return ((size_t)rows * C * sizeof(float) + 255) / 256 * 256;
}

int dvq_decode_table_prepare_f32(const float *codebook, int rows, int D, const float *conv_weight, const float *conv_bias, int C,
                                 void *table, size_t table_bytes, void *stream)
{
    const char *fn = "dvq_decode_table_prepare_f32";
    if (!codebook) { dvq_set_error("%s: null codebook", fn); return DVQ_EINVAL; }
    if (rows <= 0 || D <= 0 || C <= 0) { dvq_set_error("%s: rows=%d D=%d C=%d must be positive", fn, rows, D, C); return DVQ_EINVAL; }
    if (!conv_weight) {                                          // no conv: the codebook is the table, nothing to build
        if (conv_bias || C != D) { dvq_set_error("%s: without a conv weight there is no bias and C (%d) must equal D (%d)", fn, C, D); return DVQ_EINVAL; }
        return DVQ_OK;
    }
    if (!table) { dvq_set_error("%s: null table", fn); return DVQ_EINVAL; }
    if (D > DVQ_DECODE_MAX_C || C > DVQ_DECODE_MAX_C) { dvq_set_error("%s: D=%d / C=%d exceed %d", fn, D, C, DVQ_DECODE_MAX_C); return DVQ_EINVAL; }
    if ((size_t)rows * C >= ((size_t)1 << 40)) { dvq_set_error("%s: table too large", fn); return DVQ_EINVAL; }
    if (table_bytes < dvq_decode_table_bytes(rows, C)) { dvq_set_error("%s: table buffer %zu < %zu bytes", fn, table_bytes, dvq_decode_table_bytes(rows, C)); return DVQ_EWORKSPACE; }
    if (((uintptr_t)table & 15) != 0) { dvq_set_error("%s: table must be 16-byte aligned", fn); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_decode_table(codebook, rows, D, conv_weight, conv_bias, C, (float *)table, (hipStream_t)stream), "decode_table");
}

int dvq_decode_head_f32(const int64_t *codes, int B, int HW, const float *table, int rows, int C, const float *pos_first,
                        const float *pos_second, float *h_in, void *stream)
{
    const char *fn = "dvq_decode_head_f32";
    if (!codes || !table || !h_in) return null_pointer(fn);
    if (B <= 0 || HW <= 0 || rows <= 0 || C <= 0) { dvq_set_error("%s: B=%d HW=%d rows=%d C=%d must be positive", fn, B, HW, rows, C); return DVQ_EINVAL; }
    if (C % 4 != 0 || C > DVQ_DECODE_MAX_C) { dvq_set_error("%s: C=%d must be a multiple of 4, at most %d", fn, C, DVQ_DECODE_MAX_C); return DVQ_EINVAL; }
    if ((size_t)B * HW >= ((size_t)1 << 31) - 64 || (size_t)B * HW * C >= ((size_t)1 << 40)) { dvq_set_error("%s: tensor too large", fn); return DVQ_EINVAL; }
    if (((uintptr_t)table & 15) != 0) { dvq_set_error("%s: table must be 16-byte aligned", fn); return DVQ_EINVAL; }
    if ((((uintptr_t)h_in | (uintptr_t)pos_first | (uintptr_t)pos_second) & 3) != 0) { dvq_set_error("%s: misaligned float pointer", fn); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_decode_head((const long long *)codes, B, HW, table, rows, C, pos_first, pos_second, h_in,
                                         (hipStream_t)stream), "decode_head");
}

// ---- fused soft code assignment (vq_soft.hip) ---------------------------------------------------------------------------
size_t dvq_vq_soft_assign_workspace_bytes(int64_t N, int D, int K)
{
    if (N <= 0 || N >= ((int64_t)1 << 31) || K <= 0 || !dim_ok(D)) return 0;
    return ((size_t)N * (size_t)K * sizeof(float) + 255) / 256 * 256;
}

int dvq_vq_soft_assign_flat_f32(const float *x, const float *codebook, const void *prep, int64_t N, int D, int K, float temp,
                                const float *q, float *soft, float *dist, int64_t *codes, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_vq_soft_assign_flat_f32";
    if (!x || !codebook || !prep || !codes) return null_pointer(fn);
    if (N <= 0 || N >= ((int64_t)1 << 31) || K <= 0) { dvq_set_error("%s: N=%lld K=%d out of range", fn, (long long)N, K); return DVQ_EINVAL; }
    if (!(temp > 0.0f) || !(temp < __builtin_inff())) { dvq_set_error("%s: temp=%g must be finite and positive", fn, (double)temp); return DVQ_EINVAL; }
    if (int rc = check_width(fn, D)) return rc;
    if ((size_t)N * (size_t)K >= ((size_t)1 << 40)) { dvq_set_error("%s: N * K too large", fn); return DVQ_EUNSUPPORTED; }
    if ((((uintptr_t)x | (uintptr_t)q | (uintptr_t)soft | (uintptr_t)dist) & 3) != 0 || ((uintptr_t)prep & 255) != 0) { dvq_set_error("%s: misaligned pointer", fn); return DVQ_EINVAL; }
    float *sbuf = soft;
    if (!soft && q) {                                            // the draw alone: the scores live in the workspace
        const size_t need = dvq_vq_soft_assign_workspace_bytes(N, D, K);
        if (!ws || ws_bytes < need) { dvq_set_error("%s: workspace %zu < %zu bytes (soft == NULL with q)", fn, ws ? ws_bytes : (size_t)0, need); return DVQ_EINVAL; }
        if (int rc = check_ws_aligned(fn, ws)) return rc;
        sbuf = (float *)ws;
    }
    return hip_rc(dvq_launch_soft_assign(x, (const float *)prep, D, K, (long)N, temp, q, soft, dist, sbuf, (long long *)codes,
                                         (hipStream_t)stream), "vq_soft_assign");
}

// ---- scored / sampled assign and quantisation from given codes (vq_sample.hip) ---------------------------------------------
int dvq_vq_score_assign_f32(const float *x, const void *prep, int B, int D, int HW, int K, int metric, float temp,
                            const float *u, int64_t u_numel, int64_t *codes, void *stream)
{
    const char *fn = "dvq_vq_score_assign_f32";
    if (!x || !prep || !codes) return null_pointer(fn);
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    if (metric != DVQ_METRIC_L2 && metric != DVQ_METRIC_DOT) { dvq_set_error("%s: unknown metric %d", fn, metric); return DVQ_EINVAL; }
    if (int rc = check_width(fn, D)) return rc;
    const size_t N = (size_t)B * (size_t)HW;
    if (int rc = check_size(fn, N, true, D, K)) return rc;
    if ((((uintptr_t)x | (uintptr_t)u) & 3) != 0 || ((uintptr_t)prep & 255) != 0) { dvq_set_error("%s: misaligned pointer", fn); return DVQ_EINVAL; }
    if (u) {
        if (!(temp > 0.0f) || !(temp < __builtin_inff())) { dvq_set_error("%s: temp=%g must be finite and positive when u is given", fn, (double)temp); return DVQ_EINVAL; }
        if (u_numel < 0 || (size_t)u_numel != N * (size_t)K) { dvq_set_error("%s: u has %lld elements, expected N * K = %zu", fn, (long long)u_numel, N * (size_t)K); return DVQ_EINVAL; }
    }
    return hip_rc(dvq_launch_score_assign(x, (const float *)prep, D, HW, K, (long)N, metric, temp, u, (long long *)codes,
                                          (hipStream_t)stream), "vq_score_assign");
}

int dvq_vq_apply_codes_nchw_f32(const float *z, const int64_t *codes, const float *codebook, const float *mask, int B, int D, int HW,
                                int K, float beta, float *zq, float *loss, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_vq_apply_codes_nchw_f32";
    if (!z || !codes || !codebook) return null_pointer(fn);
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    if (D <= 0 || D % 16 != 0) { dvq_set_error("%s: D=%d must be a positive multiple of 16", fn, D); return DVQ_EUNSUPPORTED; }
    const size_t N = (size_t)B * (size_t)HW;
    if (int rc = check_size(fn, N, true, D)) return rc;
    if ((((uintptr_t)z | (uintptr_t)zq | (uintptr_t)mask) & 3) != 0 || ((uintptr_t)codebook & 15) != 0 || ((uintptr_t)codes & 7) != 0) { dvq_set_error("%s: misaligned pointer", fn); return DVQ_EINVAL; }
    if (!zq && !loss) { dvq_set_error("%s: nothing to compute (zq and loss are both null)", fn); return DVQ_EINVAL; }
    double *partials = nullptr;
    if (loss) {
        if (int rc = check_workspace(fn, ws, ws_bytes, dvq_vq_assign_workspace_bytes(B, D, HW, K, DVQ_MODE_EXACT), true)) return rc;
        partials = (double *)ws;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = dvq_launch_apply_codes(z, codebook, (const long long *)codes, mask, D, HW, K, (long)N, zq, partials, st);
    if (rc) return hip_rc(rc, "vq_apply_codes");
    if (loss) {
        rc = dvq_launch_loss_finalize(partials, dvq_apply_codes_blocks((long)N), 1.0 / ((double)N * D), beta, loss, st);
        if (rc) return hip_rc(rc, "vq_loss_finalize");
    }
    return DVQ_OK;
}

int dvq_vq_apply_codes_flat_f32(const float *z, const int64_t *codes, const float *codebook, const float *mask, int64_t N, int D,
                                int K, float beta, float *zq, float *loss, void *ws, size_t ws_bytes, void *stream)
{
    if (N <= 0 || N >= ((int64_t)1 << 31)) { dvq_set_error("dvq_vq_apply_codes_flat_f32: N=%lld out of range", (long long)N); return DVQ_EINVAL; }
    return dvq_vq_apply_codes_nchw_f32(z, codes, codebook, mask, (int)N, D, 1, K, beta, zq, loss, ws, ws_bytes, stream);
}

// ---- GumbelQuantize: projection, Gumbel argmax, KL and z_q in one sweep (vq_gumbel.hip) -----------------------------------------
size_t dvq_gumbel_prep_bytes(int K, int C)
{
    if (K <= 0 || !dim_ok(C)) return 0;
    // the f32 tile images and norms of the codebook prep, and the 256 bytes in which its builder resets the fp16 section's bound
    return (dvq_prep_f16_offset(K, C) + 255) / 256 * 256 + 256;
}

int dvq_gumbel_prepare_f32(const float *weight, const float *bias, int K, int C, void *prep, size_t prep_bytes, void *stream)
{
    const char *fn = "dvq_gumbel_prepare_f32";
    if (!weight || !prep || K <= 0) { dvq_set_error("%s: null pointer or K <= 0", fn); return DVQ_EINVAL; }
    if (!dim_ok(C)) { dvq_set_error("%s: C=%d unsupported (kernel widths 64, 128, 256)", fn, C); return DVQ_EUNSUPPORTED; }
    if (prep_bytes < dvq_gumbel_prep_bytes(K, C)) { dvq_set_error("%s: prep buffer %zu < %zu bytes", fn, prep_bytes, dvq_gumbel_prep_bytes(K, C)); return DVQ_EWORKSPACE; }
    if (((uintptr_t)prep & 255) != 0 || (((uintptr_t)weight | (uintptr_t)bias) & 3) != 0) { dvq_set_error("%s: misaligned pointer (prep: 256 bytes)", fn); return DVQ_EINVAL; }
    hipStream_t st = (hipStream_t)stream;
    int rc = dvq_launch_prep_f32(weight, K, C, prep, st);          // the codebook prep's image builder, norms in the en slot
    if (rc) return hip_rc(rc, "codebook_prep_f32");
    return hip_rc(dvq_launch_gumbel_bias(bias, K, C, prep, st), "gumbel_bias");    // ... which the bias then takes
}

size_t dvq_vq_gumbel_assign_workspace_bytes(int B, int HW)
{
    if (B <= 0 || HW <= 0) return 0;
    const size_t N = (size_t)B * (size_t)HW;
    return (((N + 127) / 128) * sizeof(double) + 255) / 256 * 256 + 256;
}

// the sweep's checked body: dvq_vq_gumbel_assign_f32 (train == false, logits == nullptr) and the training forward, which also writes the logits
static int gumbel_forward(const char *fn, bool train, const float *z, const void *prep, const float *embed, int B, int C, int HW, int K,
                          int d, float tau, float kl_K, const float *q, float *zq, int64_t *codes, float *kl, float *logits, void *ws,
                          size_t ws_bytes, void *stream)
{
    if (!z || !prep || !embed || !codes || (train && !logits)) return null_pointer(fn);
    if (B <= 0 || HW <= 0 || K <= 0 || d <= 0) { dvq_set_error("%s: B=%d HW=%d K=%d d=%d must be positive", fn, B, HW, K, d); return DVQ_EINVAL; }
    if (!dim_ok(C)) { dvq_set_error("%s: C=%d unsupported (kernel widths 64, 128, 256)", fn, C); return DVQ_EUNSUPPORTED; }
    if (q && (!(tau > 0.0f) || !(tau < __builtin_inff()))) { dvq_set_error("%s: tau=%g must be finite and positive when q is given", fn, (double)tau); return DVQ_EINVAL; }
    if (!(kl_K > 0.0f) || !(kl_K < __builtin_inff())) { dvq_set_error("%s: kl_K=%g must be finite and positive", fn, (double)kl_K); return DVQ_EINVAL; }
    const size_t N = (size_t)B * (size_t)HW;
    if (int rc = check_size(fn, N, true, C, K, d)) return rc;
    if ((((uintptr_t)z | (uintptr_t)embed | (uintptr_t)q | (uintptr_t)zq | (uintptr_t)kl | (uintptr_t)logits) & 3) != 0 || ((uintptr_t)prep & 255) != 0 || ((uintptr_t)codes & 7) != 0) { dvq_set_error("%s: misaligned pointer", fn); return DVQ_EINVAL; }
    double *partials = nullptr;
    if (kl) {
        const size_t need = dvq_vq_gumbel_assign_workspace_bytes(B, HW);
        if (!ws || ws_bytes < need) { dvq_set_error("%s: workspace %zu < %zu bytes (kl is wanted)", fn, ws ? ws_bytes : (size_t)0, need); return DVQ_EINVAL; }
        if (int rc = check_ws_aligned(fn, ws)) return rc;
        partials = (double *)ws;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = dvq_launch_gumbel_assign(z, (const float *)prep, embed, C, HW, K, d, (long)N, tau, log((double)kl_K), q, zq,
                                      (long long *)codes, partials, st, logits);
    if (rc) return hip_rc(rc, "vq_gumbel_assign");
    if (kl) {
        rc = dvq_launch_gumbel_kl_finalize(partials, dvq_gumbel_blocks((long)N), 1.0 / (double)N, kl, st);
        if (rc) return hip_rc(rc, "vq_gumbel_kl_finalize");
    }
    return DVQ_OK;
}

int dvq_vq_gumbel_assign_f32(const float *z, const void *prep, const float *embed, int B, int C, int HW, int K, int d, float tau,
                             float kl_K, const float *q, float *zq, int64_t *codes, float *kl, void *ws, size_t ws_bytes, void *stream)
{
    return gumbel_forward("dvq_vq_gumbel_assign_f32", false, z, prep, embed, B, C, HW, K, d, tau, kl_K, q, zq, codes, kl, nullptr, ws,
                          ws_bytes, stream);
}

// ---- GumbelQuantize's training step: the forward that keeps the logits, the backward down to them (vq_gumbel_backward.hip) -------
int dvq_vq_gumbel_forward_train_f32(const float *z, const void *prep, const float *embed, int B, int C, int HW, int K, int d, float tau,
                                    float kl_K, const float *q, float *zq, int64_t *codes, float *kl, float *logits, void *ws,
                                    size_t ws_bytes, void *stream)
{
    return gumbel_forward("dvq_vq_gumbel_forward_train_f32", true, z, prep, embed, B, C, HW, K, d, tau, kl_K, q, zq, codes, kl, logits,
                          ws, ws_bytes, stream);
}

int dvq_vq_gumbel_backward_f32(const float *logits, const float *q, const float *u, const float *g_kl, int B, int HW, int K, float tau,
                               float kl_K, float *dlogits, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_vq_gumbel_backward_f32";
    (void)ws; (void)ws_bytes;                                   // reserved: the kernel keeps its partial states in LDS
    if (!logits || !dlogits) return null_pointer(fn);
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    if (u && (!(tau > 0.0f) || !(tau < __builtin_inff()))) { dvq_set_error("%s: tau=%g must be finite and positive when u is given", fn, (double)tau); return DVQ_EINVAL; }
    if (g_kl && (!(kl_K > 0.0f) || !(kl_K < __builtin_inff()))) { dvq_set_error("%s: kl_K=%g must be finite and positive when g_kl is given", fn, (double)kl_K); return DVQ_EINVAL; }
    const size_t N = (size_t)B * (size_t)HW;
    if (int rc = check_size(fn, N, true, K)) return rc;
    if ((((uintptr_t)logits | (uintptr_t)q | (uintptr_t)u | (uintptr_t)g_kl | (uintptr_t)dlogits) & 3) != 0) { dvq_set_error("%s: misaligned pointer", fn); return DVQ_EINVAL; }
    // dlogits [N K] may be u itself; any other overlap with an input -- u at an offset included -- is a race between workgroups
    const uintptr_t d0 = (uintptr_t)dlogits, span = (uintptr_t)(N * (size_t)K * sizeof(float));
    auto overlaps = [&](const void *p, uintptr_t bytes) { return p && (uintptr_t)p < d0 + span && d0 < (uintptr_t)p + bytes; };
    if (overlaps(logits, span) || overlaps(q, span) || overlaps(g_kl, sizeof(float)) || (u != dlogits && overlaps(u, span))) { dvq_set_error("%s: dlogits may alias u only, and only as a whole", fn); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_gumbel_backward(logits, q, u, g_kl, HW, K, (long)N, tau, dlogits, (hipStream_t)stream), "vq_gumbel_backward");
}

// ---- narrow widths (D = 4, 8, 16): the exact VALU assign of vq_assign_narrow.hip, no prepared codebook image -----------------
size_t dvq_vq_assign_narrow_workspace_bytes(int64_t N)
{
    if (N <= 0 || N >= ((int64_t)1 << 31)) return 0;
    return ((size_t)dvq_narrow_blocks((long)N) * sizeof(double) + 255) / 256 * 256 + 256;
}

int dvq_vq_assign_narrow_tile_codes(int D) { return dvq_narrow_tile_codes(D); }

static int narrow_common(const char *fn, const float *z, const float *codebook, const float *mask, int64_t N, int D, int HW, int K,
                         bool flat, float beta, float *zq, int64_t *codes, float *loss, void *ws, size_t ws_bytes, void *stream)
{
    if (D <= 0) { dvq_set_error("%s: D=%d must be positive", fn, D); return DVQ_EINVAL; }
    if (dvq_narrow_tile_codes(D) == 0) { dvq_set_error("%s: D=%d unsupported (the narrow kernel serves the widths 4, 8 and 16; 3 runs exactly at 4 with a zero channel appended to latents and codebook; 64, 128, 256 and their zero-padded widths are dvq_vq_assign_nchw_f32's)", fn, D); return DVQ_EUNSUPPORTED; }
    if (N >= ((int64_t)1 << 31) || K >= (1 << 20)) { dvq_set_error("%s: tensor too large (N=%lld < 2^31, K=%d < 2^20)", fn, (long long)N, K); return DVQ_EUNSUPPORTED; }
    if ((((uintptr_t)z | (uintptr_t)zq | (uintptr_t)mask | (uintptr_t)loss) & 3) != 0 || ((uintptr_t)codebook & 15) != 0 || ((uintptr_t)codes & 7) != 0) { dvq_set_error("%s: misaligned pointer (codebook: 16 bytes)", fn); return DVQ_EINVAL; }
    if (flat && (((uintptr_t)z | (uintptr_t)zq) & 15) != 0) { dvq_set_error("%s: z and zq must be 16-byte aligned (rows are read and written with 16-byte accesses)", fn); return DVQ_EINVAL; }
    double *partials = nullptr;
    if (loss) {
        const size_t need = dvq_vq_assign_narrow_workspace_bytes(N);
        if (!ws || ws_bytes < need) { dvq_set_error("%s: workspace %zu < %zu bytes (loss is wanted)", fn, ws ? ws_bytes : (size_t)0, need); return DVQ_EINVAL; }
        if (int rc = check_ws_aligned(fn, ws)) return rc;
        partials = (double *)ws;
    }
    hipStream_t st = (hipStream_t)stream;
    int rc = dvq_launch_narrow(z, codebook, mask, D, HW, K, (long)N, flat, zq, (long long *)codes, partials, st);
    if (rc) return hip_rc(rc, "vq_assign_narrow");
    if (loss) {
        rc = dvq_launch_loss_finalize(partials, dvq_narrow_blocks((long)N), 1.0 / ((double)N * D), beta, loss, st);
        if (rc) return hip_rc(rc, "vq_loss_finalize");
    }
    return DVQ_OK;
}

int dvq_vq_assign_narrow_nchw_f32(const float *z, const float *codebook, const float *mask, int B, int D, int HW, int K, float beta,
                                  float *zq, int64_t *codes, float *loss, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_vq_assign_narrow_nchw_f32";
    if (!z || !codebook || !codes) return null_pointer(fn);
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    return narrow_common(fn, z, codebook, mask, (int64_t)B * HW, D, HW, K, false, beta, zq, codes, loss, ws, ws_bytes, stream);
}

int dvq_vq_assign_narrow_flat_f32(const float *z, const float *codebook, const float *mask, int64_t N, int D, int K, float beta,
                                  float *zq, int64_t *codes, float *loss, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_vq_assign_narrow_flat_f32";
    if (!z || !codebook || !codes) return null_pointer(fn);
    if (N <= 0 || K <= 0) { dvq_set_error("%s: N=%lld K=%d must be positive", fn, (long long)N, K); return DVQ_EINVAL; }
    return narrow_common(fn, z, codebook, mask, N, D, 1, K, true, beta, zq, codes, loss, ws, ws_bytes, stream);
}

// ---- the lucidrains-style codebooks: cdist-sampled assign (vq_sample.hip), orthogonal loss (ortho_loss.hip), update (ema_update.hip) ----
int dvq_vq_cdist_sample_assign_f32(const float *x, const void *prep, int B, int D, int HW, int K, float temp, const float *u,
                                   int64_t u_numel, int64_t *codes, void *stream)
{
    const char *fn = "dvq_vq_cdist_sample_assign_f32";
    if (!x || !prep || !codes || !u) { dvq_set_error("%s: null pointer (u is required: temp == 0 is the plain assign)", fn); return DVQ_EINVAL; }
    if (int rc = check_positive(fn, B, HW, K)) return rc;
    if (int rc = check_width(fn, D)) return rc;
    const size_t N = (size_t)B * (size_t)HW;
    if (int rc = check_size(fn, N, true, D, K)) return rc;
    if ((((uintptr_t)x | (uintptr_t)u) & 3) != 0 || ((uintptr_t)prep & 255) != 0) { dvq_set_error("%s: misaligned pointer", fn); return DVQ_EINVAL; }
    if (!(temp > 0.0f) || !(temp < __builtin_inff())) { dvq_set_error("%s: temp=%g must be finite and positive", fn, (double)temp); return DVQ_EINVAL; }
    if (u_numel < 0 || (size_t)u_numel != N * (size_t)K) { dvq_set_error("%s: u has %lld elements, expected N * K = %zu", fn, (long long)u_numel, N * (size_t)K); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_cdist_sample_assign(x, (const float *)prep, D, HW, K, (long)N, temp, u, (long long *)codes,
                                                 (hipStream_t)stream), "vq_cdist_sample_assign");
}

static bool ortho_shape_ok(const char *fn, int h, int n, int d)
{
    if (h <= 0 || n <= 0) { dvq_set_error("%s: h=%d n=%d must be positive", fn, h, n); return false; }
    return true;
}

size_t dvq_ortho_loss_workspace_bytes(int h, int n, int d)
{
    if (h <= 0 || n <= 0 || !dim_ok(d) || h > 65535 || n >= (1 << 24)) return 0;
    unsigned gx, gy;
    dvq_ortho_grid(h, n, &gx, &gy);
    int S, tper;
    dvq_ortho_backward_slices(h, n, &S, &tper);
    const size_t fwd = (size_t)gx * gy * (size_t)h * sizeof(double);                 // forward: one double per workgroup
    const size_t bwd = (size_t)S * (size_t)h * (size_t)n * (size_t)d * sizeof(float);   // backward: the column slices' partial gradients
    return ((fwd > bwd ? fwd : bwd) + 255) / 256 * 256;
}

int dvq_ortho_loss_forward_f32(const float *t, int h, int n, int d, float *rinv, float *loss, void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_ortho_loss_forward_f32";
    if (!t || !rinv || !loss) return null_pointer(fn);
    if (!ortho_shape_ok(fn, h, n, d)) return DVQ_EINVAL;
    if (!dim_ok(d) || h > 65535 || n >= (1 << 24)) { dvq_set_error("%s: h=%d n=%d d=%d unsupported (d in 64, 128, 256; h < 2^16, n < 2^24)", fn, h, n, d); return DVQ_EUNSUPPORTED; }
    if (((uintptr_t)t & 15) != 0 || (((uintptr_t)rinv | (uintptr_t)loss) & 3) != 0) { dvq_set_error("%s: misaligned pointer (t: 16 bytes)", fn); return DVQ_EINVAL; }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_ortho_loss_workspace_bytes(h, n, d), true)) return rc;
    return hip_rc(dvq_launch_ortho_forward(t, h, n, d, rinv, loss, (double *)ws, (hipStream_t)stream), "ortho_loss_forward");
}

int dvq_ortho_loss_backward_f32(const float *t, const float *rinv, const float *grad_out, int h, int n, int d, float *grad,
                                void *ws, size_t ws_bytes, void *stream)
{
    const char *fn = "dvq_ortho_loss_backward_f32";
    if (!t || !rinv || !grad_out || !grad) return null_pointer(fn);
    if (!ortho_shape_ok(fn, h, n, d)) return DVQ_EINVAL;
    if (!dim_ok(d) || h > 65535 || n >= (1 << 24)) { dvq_set_error("%s: h=%d n=%d d=%d unsupported (d in 64, 128, 256; h < 2^16, n < 2^24)", fn, h, n, d); return DVQ_EUNSUPPORTED; }
    if ((((uintptr_t)t | (uintptr_t)grad) & 15) != 0 || (((uintptr_t)rinv | (uintptr_t)grad_out) & 3) != 0) { dvq_set_error("%s: misaligned pointer (t, grad: 16 bytes)", fn); return DVQ_EINVAL; }
    if (t == grad) { dvq_set_error("%s: grad must not alias t", fn); return DVQ_EINVAL; }
    if (int rc = check_workspace(fn, ws, ws_bytes, dvq_ortho_loss_workspace_bytes(h, n, d), true)) return rc;
    return hip_rc(dvq_launch_ortho_backward(t, rinv, grad_out, h, n, d, grad, (float *)ws, (hipStream_t)stream), "ortho_loss_backward");
}

int dvq_lucid_update_f32(int kind, const float *counts, const float *sums, float decay, float eps, float threshold, int K, int D,
                         const float *cluster_size, float *cluster_size_out, const float *embed_avg, float *embed,
                         const float *x, int B, int HW, const int64_t *pick, void *stream)
{
    const char *fn = "dvq_lucid_update_f32";
    if (kind != 0 && kind != 1) { dvq_set_error("%s: kind must be 0 (Euclidean) or 1 (cosine), got %d", fn, kind); return DVQ_EINVAL; }
    if (!counts || !cluster_size || !cluster_size_out || !embed) return null_pointer(fn);
    if (kind == 0 && !embed_avg) { dvq_set_error("%s: kind 0 needs embed_avg", fn); return DVQ_EINVAL; }
    if (kind == 1 && !sums) { dvq_set_error("%s: kind 1 needs sums", fn); return DVQ_EINVAL; }
    if (K <= 0 || D <= 0) { dvq_set_error("%s: K=%d D=%d must be positive", fn, K, D); return DVQ_EINVAL; }
    if (cluster_size_out == cluster_size) { dvq_set_error("%s: cluster_size_out must not alias cluster_size (every workgroup reads all the OLD counts)", fn); return DVQ_EINVAL; }
    if (embed_avg == embed) { dvq_set_error("%s: embed must not alias embed_avg", fn); return DVQ_EINVAL; }
    if (!(decay >= 0.0f && decay <= 1.0f) || !(threshold >= 0.0f)) { dvq_set_error("%s: decay=%g must be in [0, 1], threshold=%g >= 0", fn, (double)decay, (double)threshold); return DVQ_EINVAL; }
    if (pick && (!x || B <= 0 || HW <= 0)) { dvq_set_error("%s: expiry (pick given) needs x [B, D, HW]", fn); return DVQ_EINVAL; }
    return hip_rc(dvq_launch_lucid_update(kind, counts, sums, decay, eps, threshold, K, D, cluster_size, cluster_size_out, embed_avg, embed,
                                          x, pick ? HW : 1, pick ? (long long)B * HW : 1, (const long long *)pick, (hipStream_t)stream),
                  "lucid_update");
}

}  // extern "C"
