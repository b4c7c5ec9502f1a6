// vq_gumbel_backward.hip -- GumbelQuantize's backward (hard / straight-through form) down to the logits, as one streaming kernel (gfx950).
//
// Replaces what autograd records for reference modules/vector_quantization/quantize_vqgan.py:171-200: the backward of the one-hot
// einsum, of F.gumbel_softmax's softmax and divide, of the second softmax, the log and the sum of the KL term -- as many passes over
// [N, K] floats as the forward made, on [N, K] tensors saved for them.  Here the saved tensors are the logits l (written by
// vq_gumbel_assign_kernel<D, NOISE, true>) and the variates q; per token n, with u_k = embed_k . G_n (a vendor GEMM of the caller):
//   s_k  = fl(fl(l_k + g_k) / tau), g_k = -logf(q_k)  (q == nullptr: fl(l_k / tau)): logf, the add and the divide in the forward's
//          order, so s has the forward's bits
//   y    = softmax(s), delta = sum_k y_k u_k;   p = softmax(l), KL_n = sum_k p_k log(p_k kl_K)
//   dl_k = y_k (u_k - delta) / tau  +  (g_kl / N) p_k (log p_k + log kl_K - KL_n)
// With the forward's state of l -- m the maximum, S = sum e^(l - m), A' = sum e^(l - m) (l - m) -- log p_k = (l_k - m) - log S and
// KL_n = A'/S - log S + log kl_K, so the second bracket is (l_k - m) - A'/S: neither log S nor kl_K is needed.  A term with
// p_k == 0 is 0 (0 log 0, as the forward); a token whose logits are all -inf, or hold a NaN, has p_k = NaN != 0 and NaN in every dl_k,
// as the torch chain has.
//
// Layout.  l, q, u, dl are [B, K, HW]: a token's codes lie K HW floats apart, consecutive tokens of an image are consecutive floats.
// A workgroup owns 32 consecutive tokens: lane (c, h), c = lane & 31, h = lane >> 5, of wave w works on token c and on the codes
// k = sl, sl + NS, sl + 2 NS, ... of slice sl = 2 w + h, NS = 2 WAVES slices -- every load and store of a lane half is 128
// contiguous bytes, the pattern of the forward's q loads.  WAVES = 4 (256 threads), or 16 (1024 threads) below 1024 workgroups,
// so that 16 384 tokens x 8192 codes are 512 workgroups of 16 waves: 8 per SIMD, 256 codes a lane.
//   pass A  per lane, in chunks of UNROLL codes whose loads are issued together: the online softmax state of s (Ms, Ss = sum e^(s - Ms),
//           Us = sum e^(s - Ms) u) and the forward's (m, S, A') of l, rescaled once per chunk at most as the forward rescales per tile;
//           chunk sums first, then added to the running sums.  While a lane has seen no finite value its exponent's base is 0, not
//           its maximum -inf: a -inf term is then 0 and a NaN stays a NaN.  The NS partial states go through LDS and every lane
//           merges its token's in the one order sl = 0 .. NS - 1, in double (the forward's combine of its two halves).
//   pass B  the same lane reads l, q, u of its codes again and writes dl.
// dlogits may be u itself: pass A has read every u of the workgroup's tokens before the barrier, in pass B a lane reads u_k and then
// writes dl_k over it, and no other workgroup touches these tokens.  (So neither pointer is __restrict__.)
// u == nullptr: no z_q gradient, the first term and q are left out; g_kl == nullptr: the second term is; both: zeros.
// g_kl is a device pointer: nothing synchronises with the host.  No atomics, vector stores only: the same bits run to run.
#include "launchers.h"

#define GB_UNROLL 8

// one partial state (max, sum, weighted sum) folded into the running one, in double, maxima in float
__device__ __forceinline__ void gb_merge(float &M, double &S, double &W, float mi, float Si, float Wi, bool second_moment)
{
    // second_moment: W is A' = sum e^(x - M) (x - M), which moves with the maximum; else W = sum e^(x - M) u, which only scales
    if (mi == -__builtin_inff()) {                   // nothing finite in the slice: its sums are 0, or NaN and stay so
        S += (double)Si;
        W += (double)Wi;
        return;
    }
    if (M == -__builtin_inff()) {                    // the first finite slice: what came before is 0 or NaN
        S += (double)Si;
        W += (double)Wi;
        M = mi;
        return;
    }
    if (mi > M) {
        const double sc = (double)expf(M - mi);
        if (second_moment) W = (W - (double)(mi - M) * S) * sc; else W = W * sc;
        S = S * sc;
        M = mi;
    }
    const double sc = (mi == M) ? 1.0 : (double)expf(mi - M);
    if (second_moment) W += ((double)Wi - (double)(M - mi) * (double)Si) * sc; else W += (double)Wi * sc;
    S += (double)Si * sc;
}

template <int WAVES, bool HAS_U, bool NOISE, bool HAS_KL>
__global__ __launch_bounds__(WAVES * 64) void vq_gumbel_backward_kernel(
    const float *__restrict__ logits, const float *__restrict__ q, const float *u, const float *__restrict__ g_kl, int HW, int K,
    long N, float tau, float *dl)
{
    constexpr int NS = 2 * WAVES;
    __shared__ float st[6][NS][32];                  // per slice and token: Ms, Ss, Us, m, S, A'

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const int sl = 2 * wave + h;
    const long n = (long)blockIdx.x * 32 + c;
    const bool valid = n < N;
    const long nn = valid ? n : N - 1;               // lanes past the end re-read the last token; they store nothing
    const long b = nn / HW;
    const size_t col = (size_t)b * (size_t)K * (size_t)HW + (size_t)(nn - b * HW);     // element k of the token: col + k HW
    const float ninf = -__builtin_inff();

    // ---- pass A
    float Ms = ninf, Ss = 0.0f, Us = 0.0f;           // of s
    float m = ninf, S = 0.0f, A = 0.0f;              // of l
    for (int k0 = sl; k0 < K; k0 += GB_UNROLL * NS) {
        float lv[GB_UNROLL], qv[GB_UNROLL], uv[GB_UNROLL];
#pragma unroll
        for (int j = 0; j < GB_UNROLL; ++j) {
            const int k = k0 + j * NS;
            const bool in = k < K;
            const size_t at = col + (size_t)(in ? k : k0) * (size_t)HW;
            lv[j] = logits[at];
            if constexpr (HAS_U && NOISE) qv[j] = q[at];
            if constexpr (HAS_U) uv[j] = u[at];
            if (!in) {
                lv[j] = ninf;
                if constexpr (HAS_U && NOISE) qv[j] = 1.0f;
                if constexpr (HAS_U) uv[j] = 0.0f;
            }
        }
        if constexpr (HAS_U) {
            float sv[GB_UNROLL], tm = ninf;
#pragma unroll
            for (int j = 0; j < GB_UNROLL; ++j) {
                sv[j] = NOISE ? __fadd_rn(lv[j], -logf(qv[j])) / tau : lv[j] / tau;
                tm = fmaxf(tm, sv[j]);               // fmaxf drops a NaN here, which reaches the sums through its own term
            }
            if (tm > Ms) {
                if (Ms != ninf) {
                    const float sc = expf(Ms - tm);
                    Ss *= sc;
                    Us *= sc;
                }
                Ms = tm;
            }
            const float base = (Ms == ninf) ? 0.0f : Ms;
            float ts = 0.0f, tu = 0.0f;
#pragma unroll
            for (int j = 0; j < GB_UNROLL; ++j) {
                const float e = expf(sv[j] - base);
                ts += e;
                tu += (e != 0.0f) ? e * uv[j] : 0.0f;
            }
            Ss += ts;
            Us += tu;
        }
        if constexpr (HAS_KL) {
            float tm = ninf;
#pragma unroll
            for (int j = 0; j < GB_UNROLL; ++j) tm = fmaxf(tm, lv[j]);
            if (tm > m) {
                if (m != ninf) {
                    const float sc = expf(m - tm);
                    A = (A - (tm - m) * S) * sc;
                    S = S * sc;
                }
                m = tm;
            }
            const float base = (m == ninf) ? 0.0f : m;
            float ts = 0.0f, ta = 0.0f;
#pragma unroll
            for (int j = 0; j < GB_UNROLL; ++j) {
                const float x = lv[j] - base;
                const float e = expf(x);
                ts += e;
                ta += (e != 0.0f) ? e * x : 0.0f;    // e == 0 (x = -inf included): the term is 0
            }
            S += ts;
            A += ta;
        }
    }
    st[0][sl][c] = Ms; st[1][sl][c] = Ss; st[2][sl][c] = Us;
    st[3][sl][c] = m;  st[4][sl][c] = S;  st[5][sl][c] = A;
    __syncthreads();

    // ---- the token's state: the slices in one fixed order
    float MsT = ninf, mT = ninf;
    double SsT = 0.0, UsT = 0.0, ST = 0.0, AT = 0.0;
    for (int i = 0; i < NS && i < K; ++i) {          // (a slice past K has no code)
        if constexpr (HAS_U) gb_merge(MsT, SsT, UsT, st[0][i][c], st[1][i][c], st[2][i][c], false);
        if constexpr (HAS_KL) gb_merge(mT, ST, AT, st[3][i][c], st[4][i][c], st[5][i][c], true);
    }
    // (reciprocals: y, p and the first term's 1 / tau are within an ulp of the quotients; s itself keeps the forward's division)
    const float inv_Ss = 1.0f / (float)SsT, delta = (float)(UsT / SsT), inv_tau = 1.0f / tau;
    const float inv_S = 1.0f / (float)ST, r = (float)(AT / ST);
    float gN = 0.0f;
    if constexpr (HAS_KL) gN = g_kl[0] / (float)N;

    // ---- pass B
    for (int k0 = sl; k0 < K; k0 += GB_UNROLL * NS) {
        float lv[GB_UNROLL], qv[GB_UNROLL], uv[GB_UNROLL];
#pragma unroll
        for (int j = 0; j < GB_UNROLL; ++j) {
            const int k = k0 + j * NS;
            const size_t at = col + (size_t)(k < K ? k : k0) * (size_t)HW;
            lv[j] = __builtin_nontemporal_load(logits + at);
            if constexpr (HAS_U && NOISE) qv[j] = __builtin_nontemporal_load(q + at);
            if constexpr (HAS_U) uv[j] = __builtin_nontemporal_load(u + at);
        }
#pragma unroll
        for (int j = 0; j < GB_UNROLL; ++j) {
            const int k = k0 + j * NS;
            float g = 0.0f;
            if constexpr (HAS_U) {
                const float s = NOISE ? __fadd_rn(lv[j], -logf(qv[j])) / tau : lv[j] / tau;
                const float y = expf(s - MsT) * inv_Ss;
                g = y * (uv[j] - delta) * inv_tau;
            }
            if constexpr (HAS_KL) {
                const float x = lv[j] - mT;
                const float p = expf(x) * inv_S;
                const float t = (p != 0.0f) ? gN * p * (x - r) : 0.0f;      // (a NaN p is not 0: the row stays NaN)
                g = HAS_U ? g + t : t;
            }
            if (valid && k < K) __builtin_nontemporal_store(g, dl + col + (size_t)k * (size_t)HW);
        }
    }
}

// u == nullptr and g_kl == nullptr: no gradient reaches the logits
__global__ __launch_bounds__(256) void vq_gumbel_backward_zero_kernel(float *__restrict__ dl, size_t count)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (size_t)gridDim.x * 256) dl[i] = 0.0f;
}

template <int WAVES>
static int launch_gumbel_backward(const float *logits, const float *q, const float *u, const float *g_kl, int HW, int K, long N,
                                  float tau, float *dl, hipStream_t st)
{
    const dim3 grid((unsigned)((N + 31) / 32)), block(WAVES * 64);
#define GB_LAUNCH(HAS_U, NOISE, HAS_KL) \
    hipLaunchKernelGGL((vq_gumbel_backward_kernel<WAVES, HAS_U, NOISE, HAS_KL>), grid, block, 0, st, logits, q, u, g_kl, HW, K, N, tau, dl)
    if (u == nullptr)            GB_LAUNCH(false, false, true);
    else if (q != nullptr) { if (g_kl != nullptr) GB_LAUNCH(true, true, true);  else GB_LAUNCH(true, true, false); }
    else                   { if (g_kl != nullptr) GB_LAUNCH(true, false, true); else GB_LAUNCH(true, false, false); }
#undef GB_LAUNCH
    return (int)hipGetLastError();
}

int dvq_launch_gumbel_backward(const float *logits, const float *q, const float *u, const float *g_kl, int HW, int K, long N,
                               float tau, float *dlogits, hipStream_t st)
{
    if (u == nullptr && g_kl == nullptr) {
        const size_t count = (size_t)N * (size_t)K;
        const size_t blocks = (count + 255) / 256;
        hipLaunchKernelGGL(vq_gumbel_backward_zero_kernel, dim3((unsigned)(blocks < 8192 ? blocks : 8192)), dim3(256), 0, st, dlogits,
                           count);
        return (int)hipGetLastError();
    }
    if ((N + 31) / 32 < 1024) return launch_gumbel_backward<16>(logits, q, u, g_kl, HW, K, N, tau, dlogits, st);
    return launch_gumbel_backward<4>(logits, q, u, g_kl, HW, K, N, tau, dlogits, st);
}
