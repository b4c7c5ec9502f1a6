// rq.hip -- residual quantization (RQBottleneck, modules/vector_quantization/quantize_rqvae.py:149-400) around the flat assign
// (gfx950).
//
// Per depth i the caller runs the flat assign on the residual r_i (codes only) and then `rq_step_kernel`, one streaming pass that
// does the reference's bookkeeping of that depth (quantize :237-271, compute_commitment_loss :283-296, forward :273-281):
//   e = E_i[c_i]   (gathered through L2: the codebook is at most 16384 x 256 x 4 B = 16 MiB)
//   agg_{i+1} = fl(agg_i + e)         (agg_0 = +0, so depth 0 gives fl(0 + e) like `zeros_like(x).add_(quant)`)
//   r_{i+1}   = fl(r_i - e)           (not on the last depth; written to the OTHER residual slot: the EMA update of depth i
//                                      reads r_i after this kernel)
//   loss partial += fl(d * d), d = fl(x - agg_{i+1})     (double per thread, fixed block order)
//   s         = fl(s + d)             (training: the commitment loss's gradient direction summed over depth)
//   codes[n, i] = c_i
// and on the last depth out = fl(x + fl(agg_d - x)) (the straight-through value) in LATENT layout instead of agg.  x is read in
// latent layout [B, H, W, Dl] through index arithmetic (to_code_shape folded into the address): code element (n, j) of token
// n = (b, hh, ww) and channel j = (a rW + c) Dl + l is latent element (b, hh rH + a, ww rW + c, l).
// These are HBM / L2 streaming kernels: 16-byte accesses where Dl % 4 == 0 and every pointer is 16-byte aligned, 4-byte ones
// otherwise.  No kernel here touches the assign's own buffers.
#include "launchers.h"
#include "../../include/dvq.h"

struct DvqRqGeom {
    unsigned h, w, rH, rW, Dl, D;   // D = rH rW Dl
    unsigned N;                     // B h w
};

// latent row (b, hh rH + a, ww rW + c) and channel l of code element (n, j)
__device__ __forceinline__ size_t rq_latent_row(const DvqRqGeom &g, unsigned n, unsigned j, unsigned &l)
{
    if (g.rH == 1 && g.rW == 1) {
        l = j;
        return n;
    }
    const unsigned hw = g.h * g.w, b = n / hw, p = n - b * hw, hh = p / g.w, ww = p - hh * g.w;
    const unsigned ac = j / g.Dl, a = ac / g.rW, c = ac - a * g.rW;
    l = j - ac * g.Dl;
    return ((size_t)b * g.h * g.rH + (size_t)hh * g.rH + a) * ((size_t)g.w * g.rW) + (size_t)ww * g.rW + c;
}

template <int VW> struct RqVec;
template <> struct RqVec<1> {
    typedef float T;
    static __device__ __forceinline__ float get(const T &v, int) { return v; }
    static __device__ __forceinline__ void set(T &v, int, float f) { v = f; }
};
template <> struct RqVec<4> {
    typedef f32x4 T;
    static __device__ __forceinline__ float get(const T &v, int k) { return v[k]; }
    static __device__ __forceinline__ void set(T &v, int k, float f) { v[k] = f; }
};

// sum of one double per thread over a 256-thread block, in a fixed order (the same bits every run)
__device__ __forceinline__ double rq_block_sum(double v)
{
    __shared__ double red[4];
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

template <int VW>
__global__ __launch_bounds__(256) void rq_step_kernel(
    const float *__restrict__ x, const float *r_in, const float *__restrict__ E, int K, const long long *__restrict__ code,
    DvqRqGeom g, int i, int depth, long long *__restrict__ codes, float *r_out, float *agg, float *s,
    float *__restrict__ out, double *__restrict__ partials)
{
    typedef typename RqVec<VW>::T V;
    const unsigned per_row = g.D / VW;
    const unsigned chunks = g.N * per_row;
    const bool first = i == 0, last = i == depth - 1;
    double sq = 0.0;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < chunks; q += gridDim.x * 256u) {
        const unsigned n = q / per_row, j = (q - n * per_row) * VW;
        const long long cn = code[n];
        const bool ok = cn >= 0 && cn < K;
        unsigned l;
        const size_t lat = rq_latent_row(g, n, j, l) * g.Dl + l;
        const size_t off = (size_t)n * g.D + j;
        const V xv = *(const V *)(x + lat);
        const V ev = ok ? *(const V *)(E + (size_t)cn * g.D + j) : V{};
        const V rv = *(const V *)(r_in + off);
        V av = first ? V{} : *(const V *)(agg + off);
        V sv = (s != nullptr && !first) ? *(const V *)(s + off) : V{};
        V rn, ov;
#pragma unroll
        for (int k = 0; k < VW; ++k) {
            const float e = ok ? RqVec<VW>::get(ev, k) : __builtin_nanf("");
            const float xe = RqVec<VW>::get(xv, k);
            const float a1 = __fadd_rn(first ? 0.0f : RqVec<VW>::get(av, k), e);
            const float d = __fsub_rn(xe, a1);
            sq += (double)__fmul_rn(d, d);
            RqVec<VW>::set(av, k, a1);
            RqVec<VW>::set(rn, k, __fsub_rn(RqVec<VW>::get(rv, k), e));
            RqVec<VW>::set(sv, k, first ? d : __fadd_rn(RqVec<VW>::get(sv, k), d));
            RqVec<VW>::set(ov, k, __fadd_rn(xe, __fsub_rn(a1, xe)));
        }
        if (s != nullptr) *(V *)(s + off) = sv;
        if (last) {
            *(V *)(out + lat) = ov;
        } else {
            *(V *)(agg + off) = av;
            *(V *)(r_out + off) = rn;
        }
        if (j == 0) codes[(size_t)n * depth + i] = cn;
    }
    const double tot = rq_block_sum(sq);
    if (threadIdx.x == 0) partials[blockIdx.x] = tot;
}

// loss = mean over depth of mean((x - agg_{i+1})^2) (compute_commitment_loss :283-296): each depth's partials summed in a fixed
// order (the vq_loss_finalize_kernel pattern), mean_i = fl(sum_i / numel), then the fp32 mean of the d means as torch.mean does it
// on a short stack: sequential sum, one division
__global__ __launch_bounds__(256) void rq_loss_kernel(const double *__restrict__ partials, int nparts, int depth, double inv_numel,
                                                      float *__restrict__ loss)
{
    __shared__ double red[256];
    float acc = 0.0f;
    for (int t = 0; t < depth; ++t) {
        double v = 0.0;
        for (int k = threadIdx.x; k < nparts; k += 256) v += partials[(size_t)t * nparts + k];
        red[threadIdx.x] = v;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
            __syncthreads();
        }
        acc = __fadd_rn(acc, (float)(red[0] * inv_numel));
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = __fdiv_rn(acc, (float)depth);
}

// g_x = fl(g_out + fl(fl(g_loss * coef) * s)), coef = fl32(2 / (numel d)): autograd's d loss / d x summed over depth, plus the
// identity of the straight-through add; written in latent layout
template <int VW>
__global__ __launch_bounds__(256) void rq_backward_kernel(const float *__restrict__ g_out, const float *__restrict__ g_loss,
                                                          float coef, DvqRqGeom g, const float *__restrict__ s,
                                                          float *__restrict__ g_x)
{
    typedef typename RqVec<VW>::T V;
    const unsigned per_row = g.D / VW;
    const unsigned chunks = g.N * per_row;
    const float c0 = (g_loss != nullptr) ? __fmul_rn(g_loss[0], coef) : 0.0f;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < chunks; q += gridDim.x * 256u) {
        const unsigned n = q / per_row, j = (q - n * per_row) * VW;
        unsigned l;
        const size_t lat = rq_latent_row(g, n, j, l) * g.Dl + l;
        const V sv = *(const V *)(s + (size_t)n * g.D + j);
        const V gv = (g_out != nullptr) ? *(const V *)(g_out + lat) : V{};
        V o;
#pragma unroll
        for (int k = 0; k < VW; ++k)
            RqVec<VW>::set(o, k, __fadd_rn(RqVec<VW>::get(gv, k), __fmul_rn(c0, RqVec<VW>::get(sv, k))));
        *(V *)(g_x + lat) = o;
    }
}

// embed_code / embed_partial_code / embed_code_with_depth (:298-369): per token the rows of codebooks 0..j (or j alone), by value
struct DvqRqBooks {
    const float *E[DVQ_RQ_MAX_DEPTH];
    int K[DVQ_RQ_MAX_DEPTH];
};

template <int VW>
__global__ __launch_bounds__(256) void rq_embed_kernel(DvqRqBooks bk, const long long *__restrict__ codes, int depth,
                                                       DvqRqGeom g, int mode, int jsel, float *__restrict__ out)
{
    typedef typename RqVec<VW>::T V;
    const unsigned per_row = g.D / VW;
    const unsigned chunks = g.N * per_row;
    const int t0 = (mode == DVQ_RQ_EMBED_SELECT) ? jsel : 0;
    const int nd = jsel + 1;
    for (unsigned q = blockIdx.x * 256u + threadIdx.x; q < chunks; q += gridDim.x * 256u) {
        const unsigned n = q / per_row, j = (q - n * per_row) * VW;
        unsigned l;
        const size_t row = rq_latent_row(g, n, j, l);
        V acc{};
        for (int t = t0; t <= jsel; ++t) {
            const long long cn = codes[(size_t)n * depth + t];
            const bool ok = cn >= 0 && cn < bk.K[t];
            V ev = ok ? *(const V *)(bk.E[t] + (size_t)cn * g.D + j) : V{};
            if (!ok)
#pragma unroll
                for (int k = 0; k < VW; ++k) RqVec<VW>::set(ev, k, __builtin_nanf(""));
            if (mode == DVQ_RQ_EMBED_EACH) {
                *(V *)(out + (row * nd + t) * g.Dl + l) = ev;
                continue;
            }
            if (mode == DVQ_RQ_EMBED_SELECT) {            // the row itself (no fl(0 + e): -0 stays -0)
                acc = ev;
                continue;
            }
#pragma unroll
            for (int k = 0; k < VW; ++k) RqVec<VW>::set(acc, k, __fadd_rn(RqVec<VW>::get(acc, k), RqVec<VW>::get(ev, k)));
        }
        if (mode != DVQ_RQ_EMBED_EACH) *(V *)(out + row * g.Dl + l) = acc;
    }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
// blocks of the step kernel, also the number of loss partials per depth: about four channels per thread, at most 2048 blocks
// (8 per CU: full occupancy for a 256-thread streaming kernel); a function of (N, D) only, so the workspace layout is
int dvq_rq_blocks(long N, int D)
{
    const long b = (N * D + 1023) / 1024;
    return (int)(b < 1 ? 1 : (b > 2048 ? 2048 : b));
}

static inline size_t rq_al(size_t b) { return (b + 255) / 256 * 256; }

// [loss partials depth x P doubles][residual slot 0][residual slot 1][agg][s (want_grad)], every section 256-byte aligned
void dvq_rq_layout(long N, int D, int depth, int want_grad, size_t *off_res0, size_t *off_res1, size_t *off_agg, size_t *off_s,
                   size_t *total)
{
    const size_t row = rq_al((size_t)N * D * sizeof(float));
    const int nres = depth - 1 < 2 ? depth - 1 : 2;
    size_t o = rq_al((size_t)depth * dvq_rq_blocks(N, D) * sizeof(double));
    *off_res0 = o;
    *off_res1 = o + (nres > 1 ? row : 0);
    o += (size_t)nres * row;
    *off_agg = o;
    o += depth > 1 ? row : 0;
    *off_s = o;
    o += want_grad ? row : 0;
    *total = o;
}

static DvqRqGeom rq_geom(int B, int h, int w, int rH, int rW, int Dl)
{
    DvqRqGeom g;
    g.h = h; g.w = w; g.rH = rH; g.rW = rW; g.Dl = Dl; g.D = rH * rW * Dl; g.N = (unsigned)B * h * w;
    return g;
}

static inline bool al16(const void *p) { return ((uintptr_t)p & 15) == 0; }

int dvq_launch_rq_step(const float *x, const float *r_in, const float *E, int K, const long long *code, int B, int h, int w,
                       int rH, int rW, int Dl, int i, int depth, int want_grad, long long *codes, float *out, void *ws,
                       hipStream_t st)
{
    const DvqRqGeom g = rq_geom(B, h, w, rH, rW, Dl);
    size_t o0, o1, oa, os, tot;
    dvq_rq_layout(g.N, g.D, depth, want_grad, &o0, &o1, &oa, &os, &tot);
    char *base = (char *)ws;
    const int P = dvq_rq_blocks(g.N, g.D);
    double *partials = (double *)base + (size_t)i * P;
    float *r_out = (float *)(base + ((i & 1) ? o1 : o0));     // r_{i+1}: slot i & 1 (r_1 -> 0, r_2 -> 1, r_3 -> 0, ...)
    float *agg = depth > 1 ? (float *)(base + oa) : nullptr;
    float *s = want_grad ? (float *)(base + os) : nullptr;
    const bool v4 = Dl % 4 == 0 && al16(x) && al16(r_in) && al16(E) && al16(out);
    if (v4)
        hipLaunchKernelGGL(rq_step_kernel<4>, dim3(P), dim3(256), 0, st, x, r_in, E, K, code, g, i, depth, codes, r_out, agg, s, out,
                           partials);
    else
        hipLaunchKernelGGL(rq_step_kernel<1>, dim3(P), dim3(256), 0, st, x, r_in, E, K, code, g, i, depth, codes, r_out, agg, s, out,
                           partials);
    return (int)hipGetLastError();
}

int dvq_launch_rq_loss(long N, int D, int depth, const void *ws, float *loss, hipStream_t st)
{
    hipLaunchKernelGGL(rq_loss_kernel, dim3(1), dim3(256), 0, st, (const double *)ws, dvq_rq_blocks(N, D), depth,
                       1.0 / ((double)N * D), loss);
    return (int)hipGetLastError();
}

int dvq_launch_rq_backward(const float *g_out, const float *g_loss, int B, int h, int w, int rH, int rW, int Dl, int depth,
                           const void *ws, float *g_x, hipStream_t st)
{
    const DvqRqGeom g = rq_geom(B, h, w, rH, rW, Dl);
    size_t o0, o1, oa, os, tot;
    dvq_rq_layout(g.N, g.D, depth, 1, &o0, &o1, &oa, &os, &tot);
    const float *s = (const float *)((const char *)ws + os);
    const float coef = (float)(2.0 / ((double)g.N * g.D * depth));
    const int P = dvq_rq_blocks(g.N, g.D);
    if (Dl % 4 == 0 && al16(g_out) && al16(g_x))
        hipLaunchKernelGGL(rq_backward_kernel<4>, dim3(P), dim3(256), 0, st, g_out, g_loss, coef, g, s, g_x);
    else
        hipLaunchKernelGGL(rq_backward_kernel<1>, dim3(P), dim3(256), 0, st, g_out, g_loss, coef, g, s, g_x);
    return (int)hipGetLastError();
}

int dvq_launch_rq_embed(const float *const *E, const int *K, int depth, const long long *codes, int B, int h, int w, int rH, int rW,
                        int Dl, int mode, int j, float *out, hipStream_t st)
{
    const DvqRqGeom g = rq_geom(B, h, w, rH, rW, Dl);
    DvqRqBooks bk = {};
    bool v4 = Dl % 4 == 0 && al16(out);
    for (int t = 0; t < depth; ++t) {
        bk.E[t] = E[t];
        bk.K[t] = K[t];
        v4 = v4 && al16(E[t]);
    }
    const int P = dvq_rq_blocks(g.N, g.D);
    if (v4)
        hipLaunchKernelGGL(rq_embed_kernel<4>, dim3(P), dim3(256), 0, st, bk, codes, depth, g, mode, j, out);
    else
        hipLaunchKernelGGL(rq_embed_kernel<1>, dim3(P), dim3(256), 0, st, bk, codes, depth, g, mode, j, out);
    return (int)hipGetLastError();
}
