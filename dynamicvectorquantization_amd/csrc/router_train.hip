// router_train.hip -- the training-mode routing tail of the dual / triple feature routers, forward and backward, for gfx950.
//
// Replaces, in training mode (differentiable into the branches and every router parameter):
//   modules/dynamic_modules/RouterDual.py:35-43, RouterTriple.py:46-56   GroupNorm per branch, AvgPool, concat, gate MLP
//   EncoderDual.py:131-156 (update_router), EncoderTriple.py:145-183     F.gumbel_softmax(hard=True), argmax, where, * gate_grad
// Forward (rt_*_fwd):
//   1. rt_pool_kernel     one pass over every branch per (image, channel group): GroupNorm (mean, rstd) and the raw per-cell
//                         averages, channel-major (the pattern of router_gate.hip's gate_pool_kernel, statistics kept apart)
//   2. rt_xbuild_kernel   cell-major gate inputs X = gamma * xhat + beta and the normalised averages XN = xhat (saved for dgamma)
//   3. rt_gemm_kernel     hidden pre-activations A = X W1^T + b1 on the fp32 matrix cores (saved; 2-layer gates only)
//   4. rt_head_kernel     per cell: logits (output layer), gumbel softmax, hard index, ret, gate_grad; saves y_soft
//   5. rt_select_kernel   h_out = where(...) * gate_grad and codebook_mask, one streaming pass
// Backward (rt_*_bwd):
//   1. rt_dgg_kernel      d gate_grad per cell = sum over channels and window of g_out * h_selected
//   2. rt_head_bwd_kernel gumbel-softmax backward -> d logits; output layer backward -> dA (act') or dX (1-layer)
//   3. rt_gemm_kernel     dX = dA W1; dW1 = dA^T X, dW2 = dl^T act(A), db = column sums (B operand of ones): split-K slabs
//      rt_slab_sum_kernel the slabs summed in slab order (no float atomics: bitwise reproducible)
//   4. rt_cellsum_kernel  per (image, feature): sum dX and sum dX * xhat over cells (fixed order), dX transposed channel-major
//   5. rt_coef_kernel     GroupNorm backward folded into dh = a1 * dX_cell + c1 * (x - mean) + c0 per (image, channel); dgamma,
//                         dbeta summed over images in image order
//   6. rt_dh_kernel       per branch one pass over its pixels: GroupNorm + pool backward plus the select's gradient
// The pool is linear and dy is constant over a pooling window, so every GroupNorm reduction is taken on cell-level tensors; only
// the final dh reads the feature maps.  All arithmetic fp32 (matrix products: v_mfma_f32_16x16x4_f32, exact fp32 products).
#include "launchers.h"

#define RT_NS_MAX 16          // split-K slabs of the reductions over cells (fixed per shape: reproducible)

struct RtLayout {
    size_t stats, pool, xn, x, apre, hh, y, kidx, gg;                 // saved by the forward
    size_t dgg, dl, da, dx, dxc, p1, p2, coef, sw1, sw2, sb1, sb2;           // backward scratch
    size_t total;
    int ns;
};

static size_t rt_a256(size_t x) { return (x + 255) / 256 * 256; }

static int rt_slabs(long N)
{
    long s = (N + 511) / 512;
    return (int)(s < 1 ? 1 : (s > RT_NS_MAX ? RT_NS_MAX : s));
}

static RtLayout rt_layout(int nb, int B, int C, int hc, int wc, int groups, int H)
{
    RtLayout L;
    const size_t ncell = (size_t)hc * wc, N = (size_t)B * ncell, F = (size_t)nb * C, G = nb;
    const size_t W2c = H > 0 ? (size_t)H : F;
    L.ns = rt_slabs((long)N);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o += rt_a256(bytes); return r; };
    L.stats = take((size_t)B * nb * (groups > 0 ? groups : 1) * 8);
    L.pool = take((size_t)B * F * ncell * 4);
    L.xn = take(groups > 0 ? N * F * 4 : 0);
    L.x = take(N * F * 4);
    L.apre = take(N * H * 4);
    L.hh = take(N * H * 4);
    L.y = take(N * G * 4);
    L.kidx = take(N * 4);
    L.gg = take(N * 4);
    L.dgg = take(N * 4);
    L.dl = take(N * G * 4);
    L.da = take(N * H * 4);
    L.dx = take(N * F * 4);
    L.dxc = take(N * F * 4);
    L.p1 = take((size_t)B * F * 4);
    L.p2 = take((size_t)B * F * 4);
    L.coef = take((size_t)B * F * 16);
    L.sw1 = take((size_t)L.ns * H * F * 4);
    L.sw2 = take((size_t)L.ns * G * W2c * 4);
    L.sb1 = take((size_t)L.ns * H * 4);
    L.sb2 = take((size_t)L.ns * G * 4);
    L.total = o;
    return L;
}

size_t dvq_route_train_ws_bytes(int nb, int B, int C, int hc, int wc, int groups, int H)
{
    return rt_layout(nb, B, C, hc, wc, groups, H).total;
}

// ---- forward 1: statistics and per-cell averages.  Workgroup = (image b, channel group g); a thread owns whole (channel, cell)
// pairs (fixed summation order), sums in double, waves combined in wave order.  groups == 0: pseudo-groups of 8, no statistics.
__global__ __launch_bounds__(256) void rt_pool_kernel(DvqRouteTrain a, float *__restrict__ pool, float2 *__restrict__ stats)
{
    const int Gp = a.groups > 0 ? a.groups : a.C / 8;
    const int cpg = a.C / Gp;
    const int b = blockIdx.x / Gp, g = blockIdx.x - b * Gp;
    const int ncell = a.hc * a.wc, F = a.nb * a.C, npair = cpg * ncell;
    __shared__ double red[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int br = 0; br < a.nb; ++br) {
        const int sc = a.nb == 2 ? (br == 0 ? 1 : 2) : (1 << br);
        const int Wb = a.wc * sc;
        const size_t plane = (size_t)(a.hc * sc) * Wb;
        const float *p0 = a.h[br] + ((size_t)b * a.C + (size_t)g * cpg) * plane;
        float *o0 = pool + ((size_t)b * F + (size_t)br * a.C + (size_t)g * cpg) * ncell;
        double s = 0.0, ss = 0.0;
        for (int pr = tid; pr < npair; pr += 256) {
            const int ch = pr / ncell, cell = pr - ch * ncell;
            const int y = cell / a.wc, x = cell - y * a.wc;
            const float *p = p0 + (size_t)ch * plane + (size_t)sc * y * Wb + sc * x;
            float v = 0.0f;
            for (int i = 0; i < sc; ++i) {
                float r = 0.0f;
                for (int j = 0; j < sc; ++j) {
                    const float t = p[(size_t)i * Wb + j];
                    s += t; ss += (double)t * t;
                    r += t;
                }
                v += r;
            }
            o0[pr] = v / (float)(sc * sc);
        }
        if (a.groups > 0) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { s += __shfl_xor(s, off); ss += __shfl_xor(ss, off); }
            __syncthreads();                                 // red[] of the previous branch consumed
            if (lane == 0) { red[0][wave] = s; red[1][wave] = ss; }
            __syncthreads();
            if (tid == 0) {
                const double n = (double)cpg * (double)plane;
                const double mean = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / n;
                double var = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / n - mean * mean;   // biased, as GroupNorm
                if (var < 0.0) var = 0.0;
                stats[((size_t)b * a.nb + br) * a.groups + g] = make_float2((float)mean, (float)(1.0 / sqrt(var + (double)a.eps)));
            }
        }
    }
}

// ---- forward 2: channel-major averages -> cell-major X (affine applied) and XN (normalised only), 32 x 32 tiles through LDS
__global__ __launch_bounds__(256) void rt_xbuild_kernel(DvqRouteTrain a, const float *__restrict__ pool,
                                                        const float2 *__restrict__ stats, float *__restrict__ X,
                                                        float *__restrict__ XN)
{
    const int ncell = a.hc * a.wc, F = a.nb * a.C;
    const int c0 = blockIdx.x * 32, k0 = blockIdx.y * 32, b = blockIdx.z;
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) {
        const int k = k0 + i, cell = c0 + tx;
        if (k < F && cell < ncell) t[i][tx] = pool[((size_t)b * F + k) * ncell + cell];
    }
    __syncthreads();
    const int k = k0 + tx;
    if (k >= F) return;
    const int br = k / a.C, ch = k - br * a.C;
    float2 st = make_float2(0.0f, 1.0f);
    float gw = 1.0f, gb = 0.0f;
    if (a.groups > 0) {
        st = stats[((size_t)b * a.nb + br) * a.groups + ch / (a.C / a.groups)];
        gw = a.gn_w[br][ch]; gb = a.gn_b[br][ch];
    }
    for (int i = ty; i < 32; i += 8) {
        const int cell = c0 + i;
        if (cell >= ncell) break;
        const size_t o = ((size_t)b * ncell + cell) * F + k;
        const float v = t[tx][i];
        if (a.groups > 0) {
            const float xn = (v - st.x) * st.y;
            XN[o] = xn;
            X[o] = xn * gw + gb;
        } else {
            X[o] = v;
        }
    }
}

// ---- fp32 matrix-core GEMM: C[m][n] (+)= sum_k A(m, k) B(k, n) (+ bias[n]); A(m, k) = AK ? A[m lda + k] : A[k lda + m],
// B(k, n) = BK ? B[n ldb + k] : B[k ldb + n], B == nullptr: all ones (column sums).  64 x 64 tile per workgroup, k-steps of 16
// through LDS, each wave a 32 x 32 quarter as 2 x 2 v_mfma_f32_16x16x4_f32 (k-ordered fma chains: the order depends on the
// shape only).  Split-K: workgroup z takes k in [z kc, (z + 1) kc) and writes slab z of C (stride slab).
template <bool AK, bool BK>
__global__ __launch_bounds__(256) void rt_gemm_kernel(int M, int N, int K, const float *__restrict__ A, long lda,
                                                      const float *__restrict__ Bm, long ldb, float *__restrict__ Cm, long ldc,
                                                      const float *__restrict__ bias, int kc, long slab)
{
    __shared__ float As[16][68], Bs[16][68];
    const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
    const int kb = blockIdx.z * kc, ke = min(K, kb + kc);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    for (int k0 = kb; k0 < ke; k0 += 16) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            int mm, kk;
            if (AK) { mm = tid >> 2; kk = (tid & 3) * 4 + q; } else { kk = tid >> 4; mm = (tid & 15) * 4 + q; }
            const int m = m0 + mm, k = k0 + kk;
            float v = 0.0f;
            if (m < M && k < ke) v = AK ? A[(size_t)m * lda + k] : A[(size_t)k * lda + m];
            As[kk][mm] = v;
            int nn;
            if (BK) { nn = tid >> 2; kk = (tid & 3) * 4 + q; } else { kk = tid >> 4; nn = (tid & 15) * 4 + q; }
            const int n = n0 + nn, k2 = k0 + kk;
            float w = 0.0f;
            if (n < N && k2 < ke) w = Bm == nullptr ? 1.0f : (BK ? Bm[(size_t)n * ldb + k2] : Bm[(size_t)k2 * ldb + n]);
            Bs[kk][nn] = w;
        }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int kr = 4 * s + (lane >> 4);
            float av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = As[kr][wm + 16 * i + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Bs[kr][wn + 16 * j + (lane & 15)];
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    float *Cz = Cm + (size_t)blockIdx.z * slab;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int n = n0 + wn + 16 * j + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + wm + 16 * i + (lane >> 4) * 4 + r;
                if (m < M && n < N) Cz[(size_t)m * ldc + n] = bias != nullptr ? acc[i][j][r] + bias[n] : acc[i][j][r];
            }
        }
}

__device__ __forceinline__ float rt_act(int act, float a)
{
    if (act == 1) return a / (1.0f + expf(-a));               // SiLU as ATen: x / (1 + exp(-x))
    if (act == 2) return a > 0.0f ? a : 0.0f;
    return a;
}

__device__ __forceinline__ float rt_dact(int act, float a)
{
    if (act == 1) {
        const float s = 1.0f / (1.0f + expf(-a));
        return s * (1.0f + a * (1.0f - s));                   // ATen's silu_backward
    }
    if (act == 2) return a > 0.0f ? 1.0f : 0.0f;
    return 1.0f;
}

// a wave-wide sum in a fixed butterfly order; every lane returns lane 0's value
__device__ __forceinline__ float rt_wave_sum(float v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return __shfl(v, 0);
}

// ---- forward 4: one wave per cell.  Output layer (over act(A) or X), then the gumbel-hard tail in the reference's rounding:
// y = softmax((logits + gumbels) / tau); k = first max of y; ret_j = (onehot_j - y_j) + y_j; indices = argmax ret; gg = ret_k.
// No gumbels: gate = logits, indices = argmax logits, gg = 1.
template <int G>
__global__ __launch_bounds__(256) void rt_head_kernel(DvqRouteTrain a, const float *__restrict__ X, const float *__restrict__ Apre,
                                                      float *__restrict__ Hh, float *__restrict__ ysave, int *__restrict__ kidx,
                                                      float *__restrict__ gg, long N)
{
    const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (cell >= N) return;
    const int F = G * a.C;
    const int W = a.hid > 0 ? a.hid : F;
    const float *src = a.hid > 0 ? Apre + (size_t)cell * W : X + (size_t)cell * W;
    float part[G];
#pragma unroll
    for (int g = 0; g < G; ++g) part[g] = 0.0f;
    for (int i = lane; i < W; i += 64) {
        float v = src[i];
        if (a.hid > 0) {
            v = rt_act(a.act, v);
            Hh[(size_t)cell * W + i] = v;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) part[g] = __builtin_fmaf(v, a.w2[(size_t)g * W + i], part[g]);
    }
    float l[G];
#pragma unroll
    for (int g = 0; g < G; ++g) l[g] = rt_wave_sum(part[g]) + a.b2[g];
    if (lane != 0) return;
    float ret[G];
    int ind = 0;
    float scale = 1.0f;
    if (a.gumbels != nullptr) {
        float z[G], m = -__builtin_inff();
#pragma unroll
        for (int g = 0; g < G; ++g) { z[g] = (l[g] + a.gumbels[(size_t)cell * G + g]) / a.tau; m = fmaxf(m, z[g]); }
        float e[G], s = 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) { e[g] = expf(z[g] - m); s += e[g]; }
        float y[G];
        int k = 0;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            y[g] = e[g] / s;
            if (y[g] > y[k]) k = g;
        }
#pragma unroll
        for (int g = 0; g < G; ++g) {
            ret[g] = ((g == k ? 1.0f : 0.0f) - y[g]) + y[g];
            ysave[(size_t)cell * G + g] = y[g];
        }
#pragma unroll
        for (int g = 1; g < G; ++g) if (ret[g] > ret[ind]) ind = g;
        scale = ret[k];
    } else {
#pragma unroll
        for (int g = 0; g < G; ++g) ret[g] = l[g];
#pragma unroll
        for (int g = 1; g < G; ++g)                          // argmax: first max, NaN wins
            if (ret[ind] == ret[ind] && (ret[g] > ret[ind] || ret[g] != ret[g])) ind = g;
    }
#pragma unroll
    for (int g = 0; g < G; ++g) a.gate[(size_t)cell * G + g] = ret[g];
    a.indices[cell] = ind;
    kidx[cell] = ind;
    gg[cell] = scale;
}

__host__ __device__ __forceinline__ int rt_scale(int nb, int br) { return nb == 2 ? (br == 0 ? 1 : 2) : (1 << br); }

// ---- forward 5: h_out[b][c][y][x] = h_sel * gg (gumbel mode) and the codebook mask (plane C of every image)
template <int G>
__global__ __launch_bounds__(256) void rt_select_kernel(DvqRouteTrain a, const int *__restrict__ kidx, const float *__restrict__ gg)
{
    const int S = G == 2 ? 2 : 4;
    const int Ho = a.hc * S, Wo = a.wc * S, ncell = a.hc * a.wc;
    const size_t plane = (size_t)Ho * Wo, total = (size_t)a.B * (a.C + 1) * plane;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pl = i / plane;
        const int r = (int)(i - pl * plane);
        const int b = (int)(pl / (a.C + 1)), c = (int)(pl - (size_t)b * (a.C + 1));
        const int y = r / Wo, x = r - y * Wo;
        const int cell = b * ncell + (y / S) * a.wc + x / S;
        const int k = kidx[cell];
        if (c == a.C) {
            const float m = G == 2 ? (k == 0 ? 0.25f : 1.0f) : (k == 0 ? 0.0625f : (k == 1 ? 0.25f : 1.0f));
            a.cmask[(size_t)b * plane + r] = m;
            continue;
        }
        const int q = S / rt_scale(G, k);                    // output pixels per source pixel edge
        const int wb = Wo / q;
        const float v = a.h[k][((size_t)b * a.C + c) * (plane / (q * q)) + (size_t)(y / q) * wb + x / q];
        a.h_out[((size_t)b * a.C + c) * plane + r] = a.gumbels != nullptr ? v * gg[cell] : v;
    }
}

// ---- backward 1: dgg[cell] = sum over channels and the cell's S x S window of g_out * h_selected (unscaled).  Workgroup = (image,
// row of cells); thread (column ox, channel lane cq) sums channels cq, cq + nq, ... in order; partials combined in cq order.
template <int G>
__global__ __launch_bounds__(256) void rt_dgg_kernel(DvqRouteTrain a, const int *__restrict__ kidx, float *__restrict__ dgg)
{
    const int S = G == 2 ? 2 : 4;
    const int Wo = a.wc * S, Ho = a.hc * S, ncell = a.hc * a.wc;
    const int b = blockIdx.x / a.hc, yc = blockIdx.x - b * a.hc;
    const int nq = Wo <= 256 ? 256 / Wo : 1;
    extern __shared__ float part[];                          // [nq][Wo]
    const size_t plane = (size_t)Ho * Wo;
    for (int t = threadIdx.x; t < nq * Wo; t += 256) {
        const int cq = t / Wo, ox = t - cq * Wo;
        const int cell = b * ncell + yc * a.wc + ox / S;
        const int k = kidx[cell];
        const int q = S / rt_scale(G, k);
        const int wb = Wo / q;
        const size_t splane = plane / (q * q);
        float acc = 0.0f;
        for (int c = cq; c < a.C; c += nq) {
            const float *go = a.g_out + ((size_t)b * a.C + c) * plane + (size_t)yc * S * Wo + ox;
            const float *hs = a.h[k] + ((size_t)b * a.C + c) * splane + (size_t)((yc * S) / q) * wb + ox / q;
            for (int dy = 0; dy < S; ++dy) acc = __builtin_fmaf(go[(size_t)dy * Wo], hs[(size_t)(dy / q) * wb], acc);
        }
        part[t] = acc;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < a.wc; x += 256) {
        float s = 0.0f;
        for (int cq = 0; cq < nq; ++cq)
            for (int d = 0; d < S; ++d) s += part[cq * Wo + x * S + d];
        dgg[b * ncell + yc * a.wc + x] = s;
    }
}

// ---- backward 2: one wave per cell.  d ret = g_gate + onehot_k dgg; dz = y (d ret - <d ret, y>); dl = dz / tau (no gumbels:
// dl = g_gate); then dA = (dl W2) * act'(A) (2-layer) or dX = dl W2 (1-layer)
template <int G>
__global__ __launch_bounds__(256) void rt_head_bwd_kernel(DvqRouteTrain a, const float *__restrict__ Apre, const float *__restrict__ ysave,
                                                          const int *__restrict__ kidx, const float *__restrict__ dgg,
                                                          float *__restrict__ dl, float *__restrict__ dA, float *__restrict__ dX, long N)
{
    const long cell = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (cell >= N) return;
    float d[G];
#pragma unroll
    for (int g = 0; g < G; ++g) d[g] = a.g_gate != nullptr ? a.g_gate[(size_t)cell * G + g] : 0.0f;
    if (a.gumbels != nullptr) {
        const int k = kidx[cell];
        const float dk = a.g_out != nullptr ? dgg[cell] : 0.0f;
        float y[G], dot = 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            if (g == k) d[g] += dk;
            y[g] = ysave[(size_t)cell * G + g];
            dot += d[g] * y[g];
        }
#pragma unroll
        for (int g = 0; g < G; ++g) d[g] = y[g] * (d[g] - dot) / a.tau;
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < G; ++g) dl[(size_t)cell * G + g] = d[g];
    }
    const int F = G * a.C;
    const int W = a.hid > 0 ? a.hid : F;
    for (int i = lane; i < W; i += 64) {
        float s = 0.0f;
#pragma unroll
        for (int g = 0; g < G; ++g) s = __builtin_fmaf(d[g], a.w2[(size_t)g * W + i], s);
        if (a.hid > 0) dA[(size_t)cell * W + i] = s * rt_dact(a.act, Apre[(size_t)cell * W + i]);
        else dX[(size_t)cell * W + i] = s;
    }
}

// out[i] = sum over slabs s = 0, 1, ... of slab[s][i]
__global__ __launch_bounds__(256) void rt_slab_sum_kernel(const float *__restrict__ slab, int ns, long len, float *__restrict__ out)
{
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < len; i += (long)gridDim.x * 256) {
        float s = slab[i];
        for (int z = 1; z < ns; ++z) s += slab[(size_t)z * len + i];
        out[i] = s;
    }
}

// ---- backward 4: workgroup = (32 features, image b): walks the image's cells in tiles of 32 (in order), P1[b][k] = sum dX,
// P2[b][k] = sum dX * xhat; the tile goes out transposed, channel-major dXc[b][k][cell]
__global__ __launch_bounds__(256) void rt_cellsum_kernel(DvqRouteTrain a, const float *__restrict__ dX, const float *__restrict__ XN,
                                                         float *__restrict__ dXc, float *__restrict__ P1, float *__restrict__ P2)
{
    const int ncell = a.hc * a.wc, F = a.nb * a.C;
    const int k0 = blockIdx.x * 32, b = blockIdx.y;
    __shared__ float t[32][33];
    __shared__ float r1[8][32], r2[8][32];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    float s1 = 0.0f, s2 = 0.0f;
    for (int c0 = 0; c0 < ncell; c0 += 32) {
        for (int i = ty; i < 32; i += 8) {
            const int cell = c0 + i, k = k0 + tx;
            float v = 0.0f, xn = 0.0f;
            if (cell < ncell && k < F) {
                const size_t o = ((size_t)b * ncell + cell) * F + k;
                v = dX[o];
                if (a.groups > 0) xn = XN[o];
            }
            s1 += v;
            s2 = __builtin_fmaf(v, xn, s2);
            t[i][tx] = v;
        }
        __syncthreads();
        for (int i = ty; i < 32; i += 8) {
            const int k = k0 + i, cell = c0 + tx;
            if (k < F && cell < ncell) dXc[((size_t)b * F + k) * ncell + cell] = t[tx][i];
        }
        __syncthreads();
    }
    r1[ty][tx] = s1; r2[ty][tx] = s2;
    __syncthreads();
    if (ty == 0 && k0 + tx < F) {
        float q1 = 0.0f, q2 = 0.0f;
        for (int j = 0; j < 8; ++j) { q1 += r1[j][tx]; q2 += r2[j][tx]; }
        P1[(size_t)b * F + k0 + tx] = q1;
        P2[(size_t)b * F + k0 + tx] = q2;
    }
}

// ---- backward 5: thread per (image, branch, group).  dx = rstd (gamma dy - S1 / n - xhat S2 / n) with dy = dX_cell / s^2 per pixel,
// S1 = sum gamma P1, S2 = sum gamma P2 over the group's channels -> coef[b][k] = (a1, c1, c0, mean): dx = a1 dX + c1 (x - mean) + c0.
// Thread per feature k (grid-stride, second part): dgamma = sum_b P2, dbeta = sum_b P1 in image order.
__global__ __launch_bounds__(256) void rt_coef_kernel(DvqRouteTrain a, const float2 *__restrict__ stats, const float *__restrict__ P1,
                                                      const float *__restrict__ P2, float4 *__restrict__ coef)
{
    const int F = a.nb * a.C;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (a.groups <= 0) {
        if (i >= a.B * F) return;
        const int k = i % F, br = k / a.C, sc = rt_scale(a.nb, br);
        coef[i] = make_float4(1.0f / (float)(sc * sc), 0.0f, 0.0f, 0.0f);
        return;
    }
    const int cpg = a.C / a.groups;
    if (i < a.B * a.nb * a.groups) {
        const int b = i / (a.nb * a.groups), r = i - b * a.nb * a.groups, br = r / a.groups, g = r - br * a.groups;
        const int sc = rt_scale(a.nb, br);
        const float2 st = stats[i];
        float S1 = 0.0f, S2 = 0.0f;
        for (int j = 0; j < cpg; ++j) {
            const int ch = g * cpg + j;
            const size_t o = (size_t)b * F + br * a.C + ch;
            const float gw = a.gn_w[br][ch];
            S1 = __builtin_fmaf(gw, P1[o], S1);
            S2 = __builtin_fmaf(gw, P2[o], S2);
        }
        const float n = (float)cpg * (float)(a.hc * sc) * (float)(a.wc * sc);
        const float c1 = -st.y * st.y * (S2 / n), c0 = -st.y * (S1 / n);
        for (int j = 0; j < cpg; ++j) {
            const int ch = g * cpg + j;
            coef[(size_t)b * F + br * a.C + ch] = make_float4(st.y * a.gn_w[br][ch] / (float)(sc * sc), c1, c0, st.x);
        }
    }
    if (i < F) {
        const int br = i / a.C, ch = i - br * a.C;
        float s1 = 0.0f, s2 = 0.0f;
        for (int b = 0; b < a.B; ++b) { s1 += P1[(size_t)b * F + i]; s2 += P2[(size_t)b * F + i]; }
        a.dgn_b[br][ch] = s1;
        a.dgn_w[br][ch] = s2;
    }
}

// ---- backward 6: dh of branch br, thread per pixel: router part a1 dXc[cell] + c1 (x - mean) + c0, plus (cell routed to br)
// the select's gradient: the sum of g_out (* gg) over the pixel's q x q output positions
template <int G>
__global__ __launch_bounds__(256) void rt_dh_kernel(DvqRouteTrain a, int br, const float *__restrict__ dXc, const float4 *__restrict__ coef,
                                                    const int *__restrict__ kidx, const float *__restrict__ gg)
{
    const int S = G == 2 ? 2 : 4;
    const int sc = rt_scale(G, br), q = S / sc;
    const int hb = a.hc * sc, wb = a.wc * sc, ncell = a.hc * a.wc, F = G * a.C, Wo = a.wc * S;
    const size_t plane = (size_t)hb * wb, oplane = plane * q * q, total = (size_t)a.B * a.C * plane;
    const float *h = a.h[br];
    float *dh = a.dh[br];
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t pl = i / plane;
        const int r = (int)(i - pl * plane);
        const int b = (int)(pl / a.C), c = (int)(pl - (size_t)b * a.C);
        const int y = r / wb, x = r - y * wb;
        const int cl = (y / sc) * a.wc + x / sc;
        const int k = br * a.C + c;
        const float4 cf = coef[(size_t)b * F + k];
        float v = cf.x * dXc[((size_t)b * F + k) * ncell + cl];
        if (a.groups > 0) v += __builtin_fmaf(cf.y, h[i] - cf.w, cf.z);
        if (a.g_out != nullptr && kidx[b * ncell + cl] == br) {
            const float s = a.gumbels != nullptr ? gg[b * ncell + cl] : 1.0f;
            const float *go = a.g_out + pl * oplane + (size_t)y * q * Wo + x * q;
            float t = 0.0f;
            for (int dy = 0; dy < q; ++dy)
                for (int dx = 0; dx < q; ++dx) t += go[(size_t)dy * Wo + dx] * s;
            v += t;
        }
        dh[i] = v;
    }
}

static int rt_grid(size_t items)
{
    size_t blocks = (items + 255) / 256;
    if (blocks > 256 * 16) blocks = 256 * 16;
    if (blocks < 1) blocks = 1;
    return (int)blocks;
}

template <bool AK, bool BK>
static void rt_gemm(int M, int N, int K, const float *A, long lda, const float *B, long ldb, float *C, long ldc, const float *bias,
                    int ns, hipStream_t st)
{
    int kc = (K + ns - 1) / ns;
    kc = (kc + 15) / 16 * 16;
    const int nz = (K + kc - 1) / kc;
    dim3 grid((N + 63) / 64, (M + 63) / 64, nz);
    hipLaunchKernelGGL((rt_gemm_kernel<AK, BK>), grid, dim3(256), 0, st, M, N, K, A, lda, B, ldb, C, ldc, bias, kc, (long)M * N);
}

// slabs of a split-K reduction over the N cells: rt_gemm with ns slabs, the unused slabs zero-filled so the sum is over a fixed count
static void rt_reduce(int M, int Ncol, long Ncells, const float *A, long lda, const float *B, long ldb, float *slab, float *out,
                      int ns, hipStream_t st)
{
    int kc = (int)((Ncells + ns - 1) / ns);
    kc = (kc + 15) / 16 * 16;
    const int nz = (int)((Ncells + kc - 1) / kc);
    rt_gemm<false, false>(M, Ncol, (int)Ncells, A, lda, B, ldb, slab, Ncol, nullptr, ns, st);
    hipLaunchKernelGGL(rt_slab_sum_kernel, dim3(rt_grid((size_t)M * Ncol)), dim3(256), 0, st, slab, nz, (long)M * Ncol, out);
}

int dvq_launch_route_train_fwd(const DvqRouteTrain *p, hipStream_t st)
{
    const DvqRouteTrain &a = *p;
    const RtLayout L = rt_layout(a.nb, a.B, a.C, a.hc, a.wc, a.groups, a.hid);
    char *ws = (char *)a.ws;
    const long N = (long)a.B * a.hc * a.wc;
    const int F = a.nb * a.C, Gp = a.groups > 0 ? a.groups : a.C / 8;
    float *pool = (float *)(ws + L.pool), *X = (float *)(ws + L.x), *XN = (float *)(ws + L.xn);
    float *Apre = (float *)(ws + L.apre), *Hh = (float *)(ws + L.hh), *y = (float *)(ws + L.y), *gg = (float *)(ws + L.gg);
    int *kidx = (int *)(ws + L.kidx);
    float2 *stats = (float2 *)(ws + L.stats);
    hipLaunchKernelGGL(rt_pool_kernel, dim3(a.B * Gp), dim3(256), 0, st, a, pool, stats);
    hipLaunchKernelGGL(rt_xbuild_kernel, dim3((a.hc * a.wc + 31) / 32, (F + 31) / 32, a.B), dim3(256), 0, st, a, pool, stats, X, XN);
    if (a.hid > 0) rt_gemm<true, true>((int)N, a.hid, F, X, F, a.w1, F, Apre, a.hid, a.b1, 1, st);
    const dim3 cg((unsigned)((N + 3) / 4));
    if (a.nb == 2) {
        hipLaunchKernelGGL(rt_head_kernel<2>, cg, dim3(256), 0, st, a, X, Apre, Hh, y, kidx, gg, N);
        hipLaunchKernelGGL(rt_select_kernel<2>, dim3(rt_grid((size_t)N * 4 * (a.C + 1))), dim3(256), 0, st, a, kidx, gg);
    } else {
        hipLaunchKernelGGL(rt_head_kernel<3>, cg, dim3(256), 0, st, a, X, Apre, Hh, y, kidx, gg, N);
        hipLaunchKernelGGL(rt_select_kernel<3>, dim3(rt_grid((size_t)N * 16 * (a.C + 1))), dim3(256), 0, st, a, kidx, gg);
    }
    return (int)hipGetLastError();
}

int dvq_launch_route_train_bwd(const DvqRouteTrain *p, hipStream_t st)
{
    const DvqRouteTrain &a = *p;
    const RtLayout L = rt_layout(a.nb, a.B, a.C, a.hc, a.wc, a.groups, a.hid);
    char *ws = (char *)a.ws;
    const long N = (long)a.B * a.hc * a.wc;
    const int F = a.nb * a.C, G = a.nb, S = a.nb == 2 ? 2 : 4;
    const float *X = (const float *)(ws + L.x), *XN = (const float *)(ws + L.xn), *Apre = (const float *)(ws + L.apre);
    const float *Hh = (const float *)(ws + L.hh), *y = (const float *)(ws + L.y), *gg = (const float *)(ws + L.gg);
    const int *kidx = (const int *)(ws + L.kidx);
    const float2 *stats = (const float2 *)(ws + L.stats);
    float *dgg = (float *)(ws + L.dgg), *dl = (float *)(ws + L.dl), *dA = (float *)(ws + L.da), *dX = (float *)(ws + L.dx);
    float *dXc = (float *)(ws + L.dxc), *P1 = (float *)(ws + L.p1), *P2 = (float *)(ws + L.p2);
    float4 *coef = (float4 *)(ws + L.coef);
    const dim3 cg((unsigned)((N + 3) / 4));
    if (a.gumbels != nullptr && a.g_out != nullptr) {
        const int Wo = a.wc * S, nq = Wo <= 256 ? 256 / Wo : 1;
        const size_t lds = (size_t)nq * Wo * sizeof(float);
        if (G == 2) hipLaunchKernelGGL(rt_dgg_kernel<2>, dim3(a.B * a.hc), dim3(256), lds, st, a, kidx, dgg);
        else hipLaunchKernelGGL(rt_dgg_kernel<3>, dim3(a.B * a.hc), dim3(256), lds, st, a, kidx, dgg);
    }
    if (G == 2) hipLaunchKernelGGL(rt_head_bwd_kernel<2>, cg, dim3(256), 0, st, a, Apre, y, kidx, dgg, dl, dA, dX, N);
    else hipLaunchKernelGGL(rt_head_bwd_kernel<3>, cg, dim3(256), 0, st, a, Apre, y, kidx, dgg, dl, dA, dX, N);
    if (a.hid > 0) {
        rt_gemm<true, false>((int)N, F, a.hid, dA, a.hid, a.w1, F, dX, F, nullptr, 1, st);            // dX = dA W1
        rt_reduce(a.hid, F, N, dA, a.hid, X, F, (float *)(ws + L.sw1), a.dw1, L.ns, st);            // dW1 = dA^T X
        rt_reduce(G, a.hid, N, dl, G, Hh, a.hid, (float *)(ws + L.sw2), a.dw2, L.ns, st);           // dW2 = dl^T act(A)
        rt_reduce(a.hid, 1, N, dA, a.hid, nullptr, 0, (float *)(ws + L.sb1), a.db1, L.ns, st);      // db1 = dA^T 1
    } else {
        rt_reduce(G, F, N, dl, G, X, F, (float *)(ws + L.sw2), a.dw2, L.ns, st);                    // dW2 = dl^T X
    }
    rt_reduce(G, 1, N, dl, G, nullptr, 0, (float *)(ws + L.sb2), a.db2, L.ns, st);                  // db2 = dl^T 1
    hipLaunchKernelGGL(rt_cellsum_kernel, dim3((F + 31) / 32, a.B), dim3(256), 0, st, a, dX, XN, dXc, P1, P2);
    const size_t nthr = (size_t)a.B * F > (size_t)F ? (size_t)a.B * F : (size_t)F;
    hipLaunchKernelGGL(rt_coef_kernel, dim3((unsigned)((nthr + 255) / 256)), dim3(256), 0, st, a, stats, P1, P2, coef);
    for (int br = 0; br < a.nb; ++br) {
        const size_t n = (size_t)N * a.C * rt_scale(a.nb, br) * rt_scale(a.nb, br);
        if (G == 2) hipLaunchKernelGGL(rt_dh_kernel<2>, dim3(rt_grid(n)), dim3(256), 0, st, a, br, dXc, coef, kidx, gg);
        else hipLaunchKernelGGL(rt_dh_kernel<3>, dim3(rt_grid(n)), dim3(256), 0, st, a, br, dXc, coef, kidx, gg);
    }
    return (int)hipGetLastError();
}
