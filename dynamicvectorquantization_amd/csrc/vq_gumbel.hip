// vq_gumbel.hip -- GumbelQuantize's forward (hard / straight-through form) as one sweep over the code tiles (gfx950).
//
// Replaces (reference modules/vector_quantization/quantize_vqgan.py:171-200): the 1x1 `proj` conv to K logits, F.gumbel_softmax
// (the Exp(1) draw's log, the add, the divide by tau, a softmax, the hard one-hot), the dense [N, K] x [K, d] einsum whose left
// operand is one-hot, a second softmax and a log for the KL term and an argmax -- about ten passes over [N, K] floats -- by ONE
// sweep that reads z and the caller-drawn variates q once and writes N codes, one scalar and z_q.  Nothing of size N x K is written.
//
// vq_gumbel_assign_kernel: built on the exact-chain tile loop's pieces (dvq_exact_tile.h; codes in rows), the tokens' C channels
// read in place from NCHW [B, C, HW] (HW == 1: row-major [N, C]).  What this kernel adds: `proj.weight` [K, C] takes the
// codebook's place in the prepared tile images, whose 32-float `en` slot holds proj.bias (dvq_gumbel_prepare_f32: the codebook
// prep's image builder, then gumbel_bias_kernel over the slot); the Gumbel argmax; the online KL state; the z_q epilogue.
//   logit   l_k = fl(dot(z_n, W_k) + b_k): the sequential-k fp32 FMA chain of the score assign, the bias added after the chain
//   code    q == nullptr: argmax_k l_k;  q given: argmax_k fl(fl(l_k + g_k) / tau), g_k = -logf(q_k), q [B, K, HW] the Exp(1)
//           variates F.gumbel_softmax draws, in the logits' own layout: the 32 lanes of a half read 128 contiguous bytes per code,
//           16 loads per lane and tile, issued before the MFMA chain that hides them.  torch.argmax's rules (argmax_take /
//           argmax_merge): the first index among equal maxima, a NaN is the maximum and the first NaN wins.
//   KL      KL_n = sum_k p_k log(p_k kl_K + 1e-10), p = softmax(l), evaluated online WITHOUT the 1e-10:
//               KL_n = A / S - m - log S + log kl_K,   m = running max, S = sum e^(l - m), A = sum e^(l - m) l.
//           Dropping the 1e-10 changes each term by p log(1 + 1e-10 / (p kl_K)) <= 1e-10 / kl_K (log(1 + x) <= x), the sum over K
//           codes by at most 1e-10 K / kl_K: 1e-10 per token when kl_K = K, against KL values of order 0.01 to 10.  A p that
//           underflows to 0 contributes 0 here and 0 log(1e-10) = 0 there.
//           The kernel carries A' = A - m S = sum e^(l - m) (l - m) (every term <= 0, none cancels against m), so that
//           KL_n = A' / S - log S + log kl_K; a lane rescales (S, A') once per tile at most, when the tile raises its maximum:
//           S <- S e^(m - m'), A' <- (A' - (m' - m) S) e^(m - m').  Tile sums are formed first and then added to the running
//           sums (two-level fp32 summation); the per-token combine and everything after it is double.  One double partial per
//           workgroup; vq_gumbel_kl_finalize_kernel adds them in one fixed order and writes kl[0] = mean_n KL_n: no atomics,
//           the same bits run to run.
//   z_q     zq[b, :, hw] = embed[code, :], the codebook row ITSELF, written once in NCHW by the kernel's epilogue (zr[] is dead by
//           then; stores of a wave cover 128-byte runs along the tokens; the rows of embed are L2-resident).  The reference's
//           value is f embed[code] with f = fl(fl(1 - y) + y), y the winner's soft probability: |f - 1| <= 2^-23.
// No atomics, no host synchronisation, vector stores only.
#include "launchers.h"
#include "dvq_exact_tile.h"

// LOGITS (the training forward, dvq_vq_gumbel_forward_train_f32): the same sweep also writes l to logits [B, K, HW], the layout of
// q -- register r of the 32 lanes of a half is one code of 32 consecutive tokens, 128 contiguous bytes per store, non-temporal (the
// backward reads them, csrc/vq_gumbel_backward.hip; nothing here does).  Everything the flag adds stands behind `if constexpr`:
// the instantiations without it are the code they were.
template <int D, bool NOISE, bool LOGITS = false>
__global__ __launch_bounds__(256, 2) void vq_gumbel_assign_kernel(
    const float *__restrict__ z, const float *__restrict__ tiles, const float *__restrict__ E, int HW, int K, int d, long N,
    float tau, double log_kl_K, const float *__restrict__ q, float *__restrict__ zq, long long *__restrict__ codes,
    double *__restrict__ partials, float *__restrict__ logits)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];   // dvq_exact_lds_bytes(D)
    __shared__ double red[4];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, h = lane >> 5;
    const long n = ((long)blockIdx.x * 4 + wave) * 32 + c;
    const bool valid = n < N;
    const long nn = valid ? n : N - 1;               // lanes past the end re-read the last token; they store nothing
    const long b = nn / HW;
    const long hw = nn - b * HW;                     // (b, hw) also address q and z_q
    float zr[D / 2];
    exact_load_token_nchw<D>(z, HW, b, nn, h, zr);

    const int T = dvq_num_tiles(K);
    exact_stage<D>(tiles, 0, lds, wave, lane);

    const bool want_kl = partials != nullptr;        // (uniform: a kernel argument)
    float best = -__builtin_inff();
    int bidx = 0x7fffffff;
    float m = -__builtin_inff(), S = 0.0f, A = 0.0f; // KL state of this lane's codes: A = sum e^(l - m) (l - m)
    const float *qcol = NOISE ? q + (size_t)b * (size_t)K * (size_t)HW + (size_t)hw : nullptr;   // q[b, k, hw] at qcol + k HW

    for (int t = 0; t < T; ++t) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                      // tile t landed; everyone is done with tile t-1
        float *buf = exact_buf<D>(lds, t);

        // this tile's variates of the lane's token: in flight under the MFMA chain
        float qq[16];
        if constexpr (NOISE) {
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int code = exact_code_of(t, g, j, h);
                    qq[4 * g + j] = (code < K) ? __builtin_nontemporal_load(qcol + (size_t)code * (size_t)HW) : 1.0f;
                }
            }
        }
        if (t + 1 < T) exact_stage<D>(tiles, t + 1, exact_buf<D>(lds, t + 1), wave, lane);

        f32x16 acc;
        exact_tile_dots<D>(buf, zr, c, h, acc);
        float l[16];
        // the row of the tile's first code of this lane half, formed behind the MFMA chain (the empty asm ties it to the chain's result:
        // formed ahead of it, the sixteen addresses would live through the chain, where the registers are fullest)
        float *lrow = nullptr;
        if constexpr (LOGITS) {
            lrow = logits + (size_t)b * (size_t)K * (size_t)HW + (size_t)hw + (size_t)exact_code_of(t, 0, 0, h) * (size_t)HW;
            asm volatile("" : "+v"(lrow) : "v"(acc[15]));
        }
        // the tile's maximum over this lane's codes: fmaxf drops a NaN here, which reaches the sums through its own term
        float tm = -__builtin_inff();
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const f32x4 b4 = exact_tile_en4<D>(buf, h, g);      // proj.bias
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int r = g * 4 + j;
                const int code = exact_code_of(t, g, j, h);
                l[r] = __fadd_rn(acc[r], b4[j]);
                if constexpr (LOGITS) {
                    if (valid && code < K) __builtin_nontemporal_store(l[r], lrow + (size_t)(j + 8 * g) * (size_t)HW);
                }
                float s = l[r];
                if constexpr (NOISE) s = __fadd_rn(s, -logf(qq[r])) / tau;
                const bool take = argmax_take(s, best) && (code < K);
                best = take ? s : best;
                bidx = take ? code : bidx;
                tm = (code < K) ? fmaxf(tm, l[r]) : tm;
            }
        }
        if (want_kl) {
            if (tm > m) {                            // rescale the running sums to the new maximum
                if (m == -__builtin_inff()) {
                    S = 0.0f; A = 0.0f;
                } else {
                    const float sc = expf(m - tm);
                    A = (A - (tm - m) * S) * sc;
                    S = S * sc;
                }
                m = tm;
            }
            float ts = 0.0f, ta = 0.0f;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int r = g * 4 + j;
                    const int code = exact_code_of(t, g, j, h);
                    const float x = l[r] - m;        // <= 0
                    const float e = (code < K) ? expf(x) : 0.0f;
                    ts += e;
                    ta += (e != 0.0f) ? e * x : 0.0f;    // e == 0 (x = -inf included): the term is 0, as 0 log(1e-10) is
                }
            }
            S += ts;
            A += ta;
        }
    }

    const int code = exact_merge_halves_argmax(best, bidx);
    if (valid && h == 0) codes[n] = (long long)code;

    if (want_kl) {
        const float m2 = __shfl_xor(m, 32), S_2 = __shfl_xor(S, 32), A_2 = __shfl_xor(A, 32);
        const float M = fmaxf(m, m2);
        auto moved = [&](float mi, float Si, float Ai, double &So, double &Ao) {   // (S, A') of one half, moved to the maximum M
            if (mi == -__builtin_inff()) { So = 0.0; Ao = 0.0; return; }        // a half without a code (K <= 4)
            const double sc = (mi == M) ? 1.0 : (double)expf(mi - M);
            Ao = ((double)Ai - (double)(M - mi) * (double)Si) * sc;
            So = (double)Si * sc;
        };
        double Sa, Aa, Sb, Ab;
        moved(m, S, A, Sa, Aa);
        moved(m2, S_2, A_2, Sb, Ab);
        const double Sd = Sa + Sb, Ad = Aa + Ab;
        double kl = (valid && h == 0) ? (Ad / Sd - log(Sd) + log_kl_K) : 0.0;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kl += __shfl_xor(kl, off);
        if (lane == 0) red[wave] = kl;
        __syncthreads();
        if (tid == 0) partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }

    // ---- z_q: the winner's row of embed, NCHW
    if (zq != nullptr && valid) {
        const float *row = E + (size_t)code * (size_t)d;
        float *op = zq + (size_t)b * (size_t)d * (size_t)HW + (size_t)hw;
        if ((d & 7) == 0 && ((uintptr_t)E & 15) == 0) {              // 16-byte pieces of the row: channels 8 s + 4 h + {0..3}
#pragma unroll 4
            for (int s = 0; s < d / 8; ++s) {
                const f32x4 e = *(const f32x4 *)(row + 8 * s + 4 * h);
#pragma unroll
                for (int j = 0; j < 4; ++j) __builtin_nontemporal_store(e[j], op + (size_t)(8 * s + 4 * h + j) * HW);
            }
        } else {
            for (int j = h; j < d; j += 2) __builtin_nontemporal_store(row[j], op + (size_t)j * HW);
        }
    }
}

// kl[0] = mean of the per-token KL terms: the partials added in one fixed order (the vq_loss_finalize_kernel pattern)
__global__ __launch_bounds__(256) void vq_gumbel_kl_finalize_kernel(const double *__restrict__ partials, int nparts, double inv_n,
                                                                     float *__restrict__ kl)
{
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 256) s += partials[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) kl[0] = (float)(red[0] * inv_n);
}

// proj.bias into the `en` slot of every tile image (0 for padded codes and for a conv without bias)
__global__ __launch_bounds__(256) void gumbel_bias_kernel(const float *__restrict__ bias, int K, int D, float *__restrict__ tiles)
{
    const int code = blockIdx.x * 256 + threadIdx.x;
    if (code >= dvq_num_tiles(K) * 32) return;
    const float v = (bias != nullptr && code < K) ? bias[code] : 0.0f;
    tiles[(size_t)(code >> 5) * dvq_tile_floats(D) + 32 * D + (code & 31)] = v;
}

int dvq_launch_gumbel_bias(const float *bias, int K, int D, void *prep, hipStream_t st)
{
    const int kpad = dvq_num_tiles(K) * 32;
    hipLaunchKernelGGL(gumbel_bias_kernel, dim3((unsigned)((kpad + 255) / 256)), dim3(256), 0, st, bias, K, D, (float *)prep);
    return (int)hipGetLastError();
}

int dvq_gumbel_blocks(long N) { return (int)((N + 127) / 128); }

template <int D>
static int launch_gumbel(const float *z, const float *tiles, const float *E, int HW, int K, int d, long N, float tau, double log_kl_K,
                         const float *q, float *zq, long long *codes, double *partials, float *logits, hipStream_t st)
{
    const size_t shmem = dvq_exact_lds_bytes(D);
    const dim3 grid((unsigned)dvq_gumbel_blocks(N)), block(256);
    if (logits != nullptr) {                         // the training forward
        if (q == nullptr)
            return dvq_launch_lds<vq_gumbel_assign_kernel<D, false, true>>(grid, block, shmem, st, z, tiles, E, HW, K, d, N, tau,
                                                                           log_kl_K, q, zq, codes, partials, logits);
        return dvq_launch_lds<vq_gumbel_assign_kernel<D, true, true>>(grid, block, shmem, st, z, tiles, E, HW, K, d, N, tau, log_kl_K,
                                                                      q, zq, codes, partials, logits);
    }
    if (q == nullptr)
        return dvq_launch_lds<vq_gumbel_assign_kernel<D, false>>(grid, block, shmem, st, z, tiles, E, HW, K, d, N, tau, log_kl_K, q, zq,
                                                                 codes, partials, logits);
    return dvq_launch_lds<vq_gumbel_assign_kernel<D, true>>(grid, block, shmem, st, z, tiles, E, HW, K, d, N, tau, log_kl_K, q, zq,
                                                            codes, partials, logits);
}

// z [B, C, HW] (HW == 1: row-major [N, C]); prep: the f32 tile images with the bias in the en slot; q nullable [B, K, HW];
// logits nullable [B, K, HW]: given, the sweep writes them too
int dvq_launch_gumbel_assign(const float *z, const float *prep, const float *E, int C, int HW, int K, int d, long N, float tau,
                             double log_kl_K, const float *q, float *zq, long long *codes, double *partials, hipStream_t st,
                             float *logits)
{
    switch (C) {
    case 64:  return launch_gumbel<64>(z, prep, E, HW, K, d, N, tau, log_kl_K, q, zq, codes, partials, logits, st);
    case 128: return launch_gumbel<128>(z, prep, E, HW, K, d, N, tau, log_kl_K, q, zq, codes, partials, logits, st);
    case 256: return launch_gumbel<256>(z, prep, E, HW, K, d, N, tau, log_kl_K, q, zq, codes, partials, logits, st);
    default:  return -1000;
    }
}

int dvq_launch_gumbel_kl_finalize(const double *partials, int nparts, double inv_n, float *kl, hipStream_t st)
{
    hipLaunchKernelGGL(vq_gumbel_kl_finalize_kernel, dim3(1), dim3(256), 0, st, partials, nparts, inv_n, kl);
    return (int)hipGetLastError();
}
